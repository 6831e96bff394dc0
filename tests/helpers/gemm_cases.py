"""Case table of the fp32 GEMM family (csrc/gemm_f32.hip, gemm_stream.hip, gemm_skinny.hip, gemm_tn.hip) and its float64 references.

One entry per (route, shape): the route the call is meant to take, its shape and strides, seeded CPU inputs, `evaluate` -- the same
operation in plain torch, in float64 for the values and in float32 for the reference's own rounding error e32 -- and the `defect`,
the float64 result with the LAST index of the reduced axis left out (the last k of an NT product, the last row r of a TN product).
Output edges need no defect: tests/test_gemm_seams_gpu.py hands every kernel a NaN-filled output, so an unwritten element fails.
Shapes sit on both sides of every seam of the launch geometry (SEAMS lists them) and are the smallest that reach it.  The inputs
make the last reduced index decisive: operands are 0.25 * randn with A[:, -1] = B[:, -1] = 2.0 (TN: the last row), so a dropped
last index moves every pre-activation output by 4.

Tolerance of a compared tensor (the GPU sweep applies it, tests/test_gemm_case_table.py proves that it sees the defect):
    primary    tol = 16 * max(e32, u * max|want|),  u = 2^-24                      (FACTOR, U: as tests/helpers/train_prim_cases.py)
    fallback   tol[m, n] = (K + 2) * u * (|A| |B|^T + |bias| + |C0 or R|)[m, n]     the a-priori bound of an fp32 sum of K products
               in any order (TN: K -> R, the reduced rows); for the cases named in FALLBACK: a kernel's fmaf chain of length K is
               legitimately less accurate than the CPU's blocked sum that e32 measures.
The host-side planning functions the routes depend on are mirrored below, each marked with the source lines it copies;
tests/test_gemm_case_table.py pins the constants they rely on to the source text.  Nothing here imports the library.
"""
import zlib

import torch

U = 2.0 ** -24
FACTOR = 16
SENSITIVITY = 10

# geometry of the kernels (pinned to csrc/ by tests/test_gemm_case_table.py)
BM, BN, BK = 128, 128, 32                   # gemm_f32.hip:24
GS_BM = 128                                 # gemm_stream.hip:20
SK_KC, SK_MAXM = 64, 128                    # gemm_skinny.hip:16
TN_RK, TN_MAXSLICES = 16, 512               # gemm_tn.hip:18,20
CUS = 256                                   # compute units of an MI355X
RESIDENT = (2 * CUS, CUS)                   # gemm_stream.hip:89 (two 64 KB workgroups per CU on gfx950); one per CU as well

ACTS = {0: 'none', 1: 'relu', 2: 'tanh', 3: 'sigmoid', 4: 'gelu', 5: 'leaky_relu', 6: 'nan_to_zero'}
ALGOS = {'auto': 0, 'tile': 1, 'stream_plain': 2, 'stream_xcd': 3, 'skinny': 4}

SEAMS = {}          # group -> {parameter: values that must appear in the table}, filled next to the cases
CASES = []
_BY_NAME = {}

# Cases whose measured error exceeds the primary rule and is judged by the a-priori bound instead (profiles/gemm_seams/measured.txt
# lists the rule and the error-to-tolerance ratio of every case).
FALLBACK = set()


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------
# mirrors of the host-side planning
def nt_kernel(M, N, K, lda, ldb, a_off=0, group=1):
    """gemm_f32.hip:332-349 (launch_gemm): which tile kernel a product runs on.  a_off: offset of A's base in floats (the
    allocations themselves are 16-byte aligned)."""
    aligned = lda % 4 == 0 and ldb % 4 == 0 and K % 4 == 0 and a_off % 4 == 0
    rows_per_tile = BM if group <= 1 else BM // group * group               # gemm_f32.hip:520 (gemm_nt_groupmax)
    fast = (aligned and group <= 1 and K % BK == 0 and K >= BK and rows_per_tile == BM and lda * 4 * BM < 2 ** 32 and
            ldb * 4 * BN < 2 ** 32)
    return 'fast' if fast else ('aligned' if aligned else 'scalar')


def fast_walk(units):
    """gemm_f32.hip:342-343 (grid) and :158-161, :175 (gemm_nt_fast_kernel's tile walk): (grid, units of the busiest XCD, trips of
    its busiest workgroup)."""
    grid = 8 * min(ceil_div(units, 8), 64)
    q, r = divmod(units, 8)
    most = q + (1 if r else 0)
    return grid, most, ceil_div(most, grid // 8)


def splitk_choice_fill(M, N, K):
    """gemm_f32.hip:384-391 (gemm_splitk_choice_fill)."""
    tiles = ceil_div(M, BM) * ceil_div(N, BN)
    if tiles >= 128 or tiles < 1 or K < 256:
        return 1
    s = min(512 // tiles, 8)
    while s > 1 and K // s < 128:
        s -= 1
    return max(s, 1)


def skinny_ok(M, N, K, lda, ldb, a_off=0):
    """gemm_skinny.hip:128-131 (gemm_skinny_ok)."""
    return 1 <= M <= SK_MAXM and N >= 16 and K >= SK_KC and K % 4 == 0 and lda % 4 == 0 and ldb % 4 == 0 and a_off % 4 == 0


def skinny_plan(M, N, K, max_slices=16):
    """gemm_skinny.hip:140-148 (gemm_skinny_partials): (16-column tiles per strip, k per slice, slices, k of the last slice)."""
    nc = 4 if (N >= 4096 or (N >= 2048 and K >= 4096)) else (2 if N >= 1024 else 1)
    col_tiles = ceil_div(N, 16 * nc)
    s = ceil_div(512 if nc > 1 else 384, col_tiles)
    s = max(1, min(s, max(K // (2 * SK_KC), 1), max_slices))
    kslice = ceil_div(ceil_div(K, s), SK_KC) * SK_KC
    ns = ceil_div(K, kslice)
    return nc, kslice, ns, K - (ns - 1) * kslice


def splitk_plan(M, N, K, lda, ldb, a_off=0):
    """gemm_f32.hip:594-617 (itr_gemm_nt_splitk with a full workspace), :420-436 (gemm_nt_splitk_fast), :393-415 (gemm_nt_splitk):
    (route, slices, k per slice, k of the last slice)."""
    if M <= 128 and N >= 16 and K >= 128 and skinny_ok(M, N, K, lda, ldb, a_off):
        nc, kslice, ns, last = skinny_plan(M, N, K)
        return 'skinny_sliced%d' % (16 * nc), ns, kslice, last
    s = splitk_choice_fill(M, N, K)
    if s <= 1:
        return 'plain_' + nt_kernel(M, N, K, lda, ldb, a_off), 1, K, K
    ksplit = ceil_div(ceil_div(K, s), BK) * BK
    ns = ceil_div(K, ksplit)
    kern = nt_kernel(M, N, K, lda, ldb, a_off)
    if kern == 'fast' and ns <= 1:
        kern = 'aligned'
    return 'splitk_' + kern, ns, ksplit, K - (ns - 1) * ksplit


def stream_plan(M, N, K, act, lda, ldb, ldc, algo, resident, a_off=0):
    """gemm_stream.hip:110-121 (gemm_nt_stream's admission test, grid and XCD map) and :44-52 (the kernel's workgroup -> row range
    split): None when the tile kernel keeps the product."""
    if algo == 1 or act not in (0, 1, 4) or K % 64 or K < 128 or N % GS_BM or M < GS_BM:
        return None
    if lda % 4 or ldb % 4 or a_off % 4 or max(lda, ldb, ldc) * 4 * GS_BM >= 2 ** 31:
        return None
    tiles_m, tiles_n = M // GS_BM, N // GS_BM
    if tiles_m * tiles_n < (0 if algo >= 2 else 2) * resident:
        return None
    grid = max(resident // tiles_n * tiles_n, tiles_n)
    xcd_map = int(algo != 2 and tiles_n >= 4 and grid % 8 == 0 and (grid // 8) % tiles_n == 0)
    nw = grid // tiles_n
    q, r = divmod(tiles_m, nw)
    return {'grid': grid, 'xcd_map': xcd_map, 'tiles_m': tiles_m, 'tiles_n': tiles_n, 'nw': nw, 'q': q, 'r': r,
            'idle': nw - r if q == 0 else 0, 'rest': M - tiles_m * GS_BM, 'nk2': K // 64}


def nt_algo_route(M, N, K, act, lda, ldb, ldc, algo, resident=RESIDENT[0], a_off=0):
    """gemm_f32.hip:472-492 (gemm_nt_algo)."""
    if algo == 4:
        if N >= 64 and K >= 128 and skinny_ok(M, N, K, lda, ldb, a_off):
            return 'skinny_direct'
        algo = 0
    p = stream_plan(M, N, K, act, lda, ldb, ldc, algo, resident, a_off)
    if p:
        return 'stream_xcd' if p['xcd_map'] else 'stream_plain'
    return nt_kernel(M, N, K, lda, ldb, a_off)


def tn_tile(P, Q):
    """gemm_tn.hip:182-185 (tn_tile)."""
    m = min(P, Q)
    return 128 if m > 64 else (64 if m > 32 else 32)


def tn_plan(R, P, Q):
    """gemm_tn.hip:186-199 (tn_plan): (tile, slices, rows per slice, rows of the last slice)."""
    T = tn_tile(P, Q)
    tiles = ceil_div(P, T) * ceil_div(Q, T)
    s = max(1, min(ceil_div(1024, tiles), ceil_div(R, 256), TN_MAXSLICES))
    rps = max(ceil_div(ceil_div(R, s), TN_RK) * TN_RK, TN_RK)
    nsl = ceil_div(R, rps) if R > 0 else 1
    return T, nsl, rps, R - (nsl - 1) * rps


def tn_aligned(lda, ldb, P, Q, a_off=0, b_off=0, batch_a=0, batch_b=0):
    """gemm_tn.hip:222-223 (gemm_tn) and :250-251 (gemm_tn_batched)."""
    return all(v % 4 == 0 for v in (lda, ldb, P, Q, a_off, b_off, batch_a, batch_b))


def tn_rows_for(nsl, P, Q):
    """The smallest R that tn_plan cuts into `nsl` slices with a short last one."""
    for R in range(1, 1 << 16):
        _, n, rps, last = tn_plan(R, P, Q)
        if n == nsl and (last < rps or nsl == 1):
            return R
    raise ValueError((nsl, P, Q))


# ---------------------------------------------------------------------------------------------------------------------
def _act(v, code):
    if code == 1:
        return torch.relu(v)
    if code == 2:
        return torch.tanh(v)
    if code == 3:
        return torch.sigmoid(v)
    if code == 4:
        return torch.nn.functional.gelu(v)
    if code == 5:
        return torch.where(v > 0, v, 0.1 * v)
    if code == 6:
        return torch.where(v != v, torch.zeros_like(v), v)
    return v


class Case(object):
    """kind 'nt': C[M, N] = act(A B^T + bias (+ C0 | + R)), A's row m at a_off + m * lda of one flat buffer (rows may overlap);
    'groupmax': S[Ni, Nc] = max over k views of img[Ni, k, D] . cap[Nc, D]; 'tn': C[P, Q] (+)= A[R, P]^T B[R, Q], A and B column
    windows a_off / b_off of wider matrices; 'tn_batched': `batch` TN products at batch strides batch_a / batch_b."""
    DEFAULTS = {
        'nt': dict(lda=None, ldc=None, ldr=None, a_off=0, act=0, bias=0, algo='auto', nan=0),
        'groupmax': dict(ldc=None),
        'tn': dict(lda=None, ldb=None, ldc=None, a_off=0, b_off=0, acc=0, colsum=0),
        'tn_batched': dict(pad_a=0, pad_b=0),
    }

    def __init__(self, group, kind, entry, route, **shape):
        self.group, self.kind, self.entry, self.route = group, kind, entry, route
        self.name = "%s-%s-%s" % (group, entry, "-".join("%s%s" % (k, v) for k, v in shape.items()))
        s = dict(self.DEFAULTS[kind])
        s.update(shape)
        if kind == 'nt':
            s['lda'] = s['K'] if s['lda'] is None else s['lda']
            s['ldc'] = s['N'] if s['ldc'] is None else s['ldc']
            s['ldr'] = s['N'] if s['ldr'] is None else s['ldr']
        elif kind == 'groupmax':
            s['M'], s['N'], s['K'] = s['Ni'] * s['k'], s['Nc'], s['D']
            s['ldc'] = s['Nc'] if s['ldc'] is None else s['ldc']
        elif kind == 'tn':
            s['lda'] = s['P'] + s['a_off'] if s['lda'] is None else s['lda']
            s['ldb'] = s['Q'] + s['b_off'] if s['ldb'] is None else s['ldb']
            s['ldc'] = s['Q'] if s['ldc'] is None else s['ldc']
        else:
            s['batch_a'], s['batch_b'] = s['R'] * s['P'] + s['pad_a'], s['R'] * s['Q'] + s['pad_b']
        self.shape = s
        self.plan = self._plan()

    def __repr__(self):
        return self.name

    @property
    def rule(self):
        return 'fallback' if self.name in FALLBACK else 'primary'

    @property
    def reduced(self):
        return self.shape['R'] if self.kind in ('tn', 'tn_batched') else self.shape['K']

    # ---- where the mirrors put the call --------------------------------------------------------------------------
    def _plan(self):
        s = self.shape
        p = {}
        if self.kind == 'groupmax':
            p['route'] = 'groupmax_' + nt_kernel(s['M'], s['N'], s['K'], s['K'], s['K'], 0, s['k'])
            p['rows_per_tile'] = BM if s['k'] <= 1 else BM // s['k'] * s['k']
            p['row_tiles'] = ceil_div(s['M'], p['rows_per_tile'])
        elif self.kind == 'nt':
            M, N, K, lda, ldc, a_off = s['M'], s['N'], s['K'], s['lda'], s['ldc'], s['a_off']
            p['tiles'] = ceil_div(M, BM) * ceil_div(N, BN)
            if self.entry == 'splitk':
                p['route'], p['ns'], p['kslice'], p['last'] = splitk_plan(M, N, K, lda, K, a_off)
                p['last_full'] = int(p['last'] == p['kslice'])
                if p['route'].startswith('plain_'):                 # not sliced: gemm_nt's automatic route
                    p['route'] = 'plain_' + nt_algo_route(M, N, K, s['act'], lda, K, ldc, 0, RESIDENT[0], a_off)
                if p['route'] == 'splitk_fast':
                    p['walk'] = fast_walk(p['tiles'] * p['ns'])
            elif self.entry == 'algo':
                algo = ALGOS[s['algo']]
                p['route'] = nt_algo_route(M, N, K, s['act'], lda, K, ldc, algo, RESIDENT[0], a_off)
                if p['route'].startswith('stream'):
                    for res in RESIDENT:
                        sp = stream_plan(M, N, K, s['act'], lda, K, ldc, algo, res, a_off)
                        p['stream@%d' % res] = sp
                        W = res // sp['tiles_n']
                        label = {1: '1', W - 1: 'W-1', W: 'W', W + 1: 'W+1', 2 * W + 1: '2W+1'}.get(sp['tiles_m'])
                        p['tn:tm@%d' % res] = '%d:%s' % (sp['tiles_n'], label)
                    p['tiles_n'], p['nk2'], p['rest'] = N // GS_BM, K // 64, M % GS_BM
            else:       # 'nt' (itr_gemm_nt: the automatic route), 'acc', 'residual' (launch_gemm directly)
                auto = nt_algo_route(M, N, K, s['act'], lda, K, ldc, 0, RESIDENT[0], a_off)
                p['route'] = auto if self.entry == 'nt' else nt_kernel(M, N, K, lda, K, a_off)
            if p['route'] == 'fast':
                p['nk'] = K // BK
                p['walk'] = fast_walk(p['tiles'])
            if self.entry == 'algo' and p['route'] == 'skinny_direct':
                p['row_tiles'] = ceil_div(M, 16)
        elif self.kind == 'tn':
            T, nsl, rps, last = tn_plan(s['R'], s['P'], s['Q'])
            al = tn_aligned(s['lda'], s['ldb'], s['P'], s['Q'], s['a_off'], s['b_off'])
            p.update(route='tn%d_%s' % (T, 'aligned' if al else 'scalar'), T=T, nsl=nsl, rps=rps, last=last, minPQ=min(s['P'], s['Q']),
                     direct=int(nsl == 1 and not s['acc']), last_short=int(nsl > 1 and last < rps))
        else:
            T = tn_tile(s['P'], s['Q'])
            al = tn_aligned(s['P'], s['Q'], s['P'], s['Q'], 0, 0, s['batch_a'], s['batch_b'])
            p.update(route='tnb%d_%s' % (T, 'aligned' if al else 'scalar'), T=T, minPQ=min(s['P'], s['Q']))
        return p

    # ---- inputs and references ---------------------------------------------------------------------------------
    def inputs(self):
        """Seeded float32 CPU tensors.  'abuf' / 'A' etc. are the buffers the kernel reads; 'Av' / 'Bv' the operand views."""
        g = torch.Generator().manual_seed(zlib.crc32(self.name.encode()))
        s = self.shape
        x = {}

        def rn(*shape):
            return 0.25 * torch.randn(*shape, generator=g)

        if self.kind == 'nt':
            M, N, K, lda, a_off = s['M'], s['N'], s['K'], s['lda'], s['a_off']
            buf = rn(max(a_off + (M - 1) * lda + K, 4))
            B = rn(N, max(K, 1))[:, :K].contiguous() if K == 0 else rn(N, K)
            if K:
                buf[a_off + torch.arange(M) * lda + K - 1] = 2.0
                B[:, K - 1] = 2.0
            if s['nan']:                                                # a NaN in the FIRST k of the last row: act 6 zeroes that row
                buf[a_off + (M - 1) * lda] = float('nan')
            x.update(abuf=buf, B=B, Av=torch.as_strided(buf, (M, K), (lda, 1), a_off), Bv=B)
            if s['bias']:
                x['bias'] = torch.randn(N, generator=g)
            if self.entry in ('acc', 'residual'):
                x['C0'] = torch.randn(M, N, generator=g)
        elif self.kind == 'groupmax':
            img, cap = rn(s['Ni'], s['k'], s['D']), rn(s['Nc'], s['D'])
            img[:, :, -1] = 2.0
            cap[:, -1] = 2.0
            x.update(img=img, cap=cap, Av=img.view(-1, s['D']), Bv=cap)
        elif self.kind == 'tn':
            R, P, Q = s['R'], s['P'], s['Q']
            A, B = rn(R, s['lda']), rn(R, s['ldb'])
            if R:
                A[-1] = 2.0
                B[-1] = 2.0
            x.update(A=A, B=B, Av=A[:, s['a_off']:s['a_off'] + P], Bv=B[:, s['b_off']:s['b_off'] + Q])
            if s['acc']:
                x['C0'] = torch.randn(P, Q, generator=g)
        else:
            Bn, R, P, Q = s['batch'], s['R'], s['P'], s['Q']
            A, B = rn(Bn, s['batch_a']), rn(Bn, s['batch_b'])
            Av, Bv = A[:, :R * P].view(Bn, R, P), B[:, :R * Q].view(Bn, R, Q)
            if R:
                Av[:, -1] = 2.0
                Bv[:, -1] = 2.0
            x.update(A=A, B=B, Av=Av, Bv=Bv)
        return x

    def evaluate(self, x, dtype, drop=0, absolute=False):
        """{tensor: value} in `dtype` with the last `drop` indices of the reduced axis left out; absolute: the sum of the absolute
        values of every term instead (before the activation), for the a-priori bound."""
        s = self.shape

        def cv(t):
            t = t.to(dtype)
            return t.abs() if absolute else t

        A, B = cv(x['Av']), cv(x['Bv'])
        if self.kind in ('nt', 'groupmax'):
            K = s['K'] - drop
            pre = A[:, :K] @ B[:, :K].t()
            if 'bias' in x:
                pre = pre + cv(x['bias'])
            if 'C0' in x:
                pre = pre + cv(x['C0'])
            if self.kind == 'groupmax':
                return {'C': pre.view(s['Ni'], s['k'], s['Nc']).max(1).values}
            return {'C': pre if absolute else _act(pre, s['act'])}
        R = s['R'] - drop
        if self.kind == 'tn':
            out = {'C': A[:R].t() @ B[:R] + (cv(x['C0']) if 'C0' in x else 0)}
            if s['colsum']:
                out['colsum'] = A[:R].sum(0)
            return out
        return {'C': torch.bmm(A[:, :R].transpose(1, 2), B[:, :R])}

    def reference(self, x=None):
        """{tensor: (want float64, e32, primary tol)}."""
        x = self.inputs() if x is None else x
        w64, w32 = self.evaluate(x, torch.float64), self.evaluate(x, torch.float32)
        out = {}
        for k, want in w64.items():
            e32 = float((w32[k].double() - want).abs().max()) if want.numel() else 0.0
            out[k] = (want, e32, FACTOR * max(e32, U * (float(want.abs().max()) if want.numel() else 0.0)))
        return out

    def fallback(self, x=None):
        """{tensor: elementwise float64 bound (n + 2) u (sum of the terms' absolute values)}, n the length of the reduced axis."""
        x = self.inputs() if x is None else x
        return {k: (self.reduced + 2) * U * v for k, v in self.evaluate(x, torch.float64, absolute=True).items()}

    def defect(self, x=None):
        """{tensor: float64 result without the last index of the reduced axis}; None where nothing is reduced."""
        if self.reduced == 0:
            return None
        return self.evaluate(self.inputs() if x is None else x, torch.float64, drop=1)


def _add(group, kind, entry, route, **shape):
    c = Case(group, kind, entry, route, **shape)
    assert c.name not in _BY_NAME, c.name
    CASES.append(c)
    _BY_NAME[c.name] = c
    return c


def cases(*groups):
    return [c for c in CASES if c.group in groups]


def _seam(group, **params):
    SEAMS.setdefault(group, {}).update({k: sorted(set(v), key=str) for k, v in params.items()})


# ---------------------------------------------------------------------------------------------------------------------
# NT tile kernels: M x N over both sides of a tile, K over the generated loop's prologue and tails (fast), the float4 path
# (aligned) and the scalar path; bias and activation rotate through the table
EDGE = (1, 127, 128, 129, 257)
TILE_K = {'fast': (32, 64, 96, 128, 160), 'aligned': (4, 36, 100), 'scalar': (1, 6, 37)}
_n = 0
for _kern, _ks in TILE_K.items():
    for _K in _ks:
        for _M in EDGE:
            for _N in EDGE:
                _add('tile_' + _kern, 'nt', 'algo', _kern, M=_M, N=_N, K=_K, algo='tile', bias=_n % 2, act=(0, 1, 4, 5)[_n // 2 % 4])
                _n += 1
    _seam('tile_' + _kern, M=EDGE, N=EDGE, K=_ks, bias=(0, 1))
_seam('tile_fast', nk=(1, 2, 3, 4, 5))

# tile counts of the persistent walk (8 XCD ranges, 64 slots each) and of the generic kernel's XCD remap: 1, 7, 8, 9 and 23 x 23
TILE_COUNTS = {1: (128, 128), 7: (769, 100), 8: (1024, 128), 9: (300, 300), 529: (2817, 2817)}
for _t, (_M, _N) in TILE_COUNTS.items():
    _add('tile_count', 'nt', 'algo', 'fast', M=_M, N=_N, K=32, algo='tile', bias=1)
    _add('tile_count', 'nt', 'algo', 'aligned', M=_M, N=_N, K=4, algo='tile')
_seam('tile_count', tiles=TILE_COUNTS)

# epilogues: every activation code with and without bias on each kernel; code 6 through itr_gemm_nt; accumulate; residual
EPI_K = {'fast': 64, 'aligned': 36, 'scalar': 37}
for _kern, _K in EPI_K.items():
    for _a in range(6):
        for _b in (0, 1):
            _add('epilogue', 'nt', 'algo', _kern, M=129, N=130, K=_K, algo='tile', act=_a, bias=_b)
    _add('epilogue', 'nt', 'nt', _kern, M=129, N=130, K=_K, act=6, bias=1, nan=1)
    for _a in (0, 1, 3):
        _add('epilogue', 'nt', 'acc', _kern, M=129, N=257, K=_K, act=_a, bias=_a % 2, ldc=257 + 3 * _a)
        _add('epilogue', 'nt', 'residual', _kern, M=129, N=257, K=_K, act=_a, bias=1 - _a % 2, ldr=260 + _a, ldc=257 + 2 * _a)
_seam('epilogue', act=range(7), bias=(0, 1))

# strides: ldc > N (guard columns), lda > K, lda < K (overlapping rows), a 4-byte-offset base, K = 0
for _kern, _K, _lda in (('fast', 64, 96), ('fast', 64, 32), ('fast', 96, 4), ('aligned', 36, 40), ('aligned', 36, 4), ('scalar', 64, 65),
                        ('scalar', 37, 3), ('scalar', 37, 41), ('scalar', 64, 62)):
    _add('strides', 'nt', 'nt', _kern, M=257, N=129, K=_K, lda=_lda, ldc=133, bias=1)
_add('strides', 'nt', 'nt', 'scalar', M=257, N=129, K=64, a_off=1, ldc=130)
_add('strides', 'nt', 'nt', 'scalar', M=129, N=257, K=64, a_off=1, lda=68, ldc=259, bias=1, act=1)
for _a in (0, 3):                                      # K = 0: C = act(bias)
    _add('strides', 'nt', 'nt', 'aligned', M=129, N=130, K=0, lda=4, act=_a, bias=1, ldc=131)
_add('strides', 'nt', 'nt', 'scalar', M=129, N=130, K=0, lda=1)
_seam('strides', K=(0, 36, 37, 64), a_off=(0, 1))

# ---------------------------------------------------------------------------------------------------------------------
# group-max epilogue (itr_mvm_scores): rows_per_tile = (128 / k) k; Ni on both sides of one row tile; D % 4 == 0 or not
MVM_K = (1, 2, 3, 12, 37, 64, 65, 128)
MVM_NC = (127, 128, 129)
MVM_D = (8, 7)
for _k in MVM_K:
    _g = 128 // _k
    for _Ni in sorted(set((max(_g - 1, 1), _g, _g + 1))):
        for _Nc in MVM_NC:
            for _D in MVM_D:
                _add('groupmax', 'groupmax', 'mvm', 'groupmax_' + ('aligned' if _D % 4 == 0 else 'scalar'), Ni=_Ni, k=_k, Nc=_Nc, D=_D)
_add('groupmax', 'groupmax', 'mvm', 'groupmax_fast', Ni=129, k=1, Nc=129, D=32)           # one view: the plain kernel
_add('groupmax', 'groupmax', 'mvm', 'groupmax_aligned', Ni=5, k=37, Nc=129, D=32, ldc=131)
_seam('groupmax', k=MVM_K, Nc=MVM_NC, D=MVM_D, rows_per_tile=(128, 126, 120, 111, 65), row_tiles=(1, 2))

# ---------------------------------------------------------------------------------------------------------------------
# streaming kernel, forced (the two-round rule waived): W = resident workgroups / tiles_n row ranges
STREAM_TN = (1, 3, 4, 8)
STREAM_K = (128, 192, 256, 320)
STREAM_ACT = (0, 1, 4)
STREAM_TM = ('1', 'W-1', 'W', 'W+1', '2W+1')
_n = 0
for _tn in STREAM_TN:           # one case per shape: the GPU sweep runs it on the tile kernel and on both maps of the streaming kernel
    _tms = set([1])
    for _res in RESIDENT:
        _W = _res // _tn
        _tms |= set((_W - 1, _W, _W + 1, 2 * _W + 1))
    for _tm in sorted(_tms):
        _add('stream', 'nt', 'algo', 'stream_xcd' if _tn >= 4 else 'stream_plain', M=_tm * 128 + (5 if _n // 2 % 2 else 0), N=_tn * 128,
             K=STREAM_K[_n % 4] if _tm <= 512 else 128, algo='stream_xcd', act=STREAM_ACT[_n % 3], bias=(_n // 3) % 2)
        _n += 1
_add('stream', 'nt', 'algo', 'stream_xcd', M=3 * 128 + 5, N=512, K=128, algo='stream_xcd', ldc=516, bias=1, act=1)
_add('stream', 'nt', 'algo', 'stream_plain', M=3 * 128, N=384, K=256, algo='stream_xcd', lda=64, bias=1)
_add('stream', 'nt', 'algo', 'stream_xcd', M=5 * 128, N=1024, K=192, algo='stream_xcd', lda=128, ldc=1028, act=4)
_seam('stream', tiles_n=STREAM_TN, nk2=(2, 3, 4, 5), act=STREAM_ACT, bias=(0, 1), rest=(0, 5),
      **{'tn:tm@%d' % _res: ['%d:%s' % (_tn, _l) for _tn in STREAM_TN for _l in STREAM_TM] for _res in RESIDENT})

# ---------------------------------------------------------------------------------------------------------------------
# split-K through itr_gemm_nt_splitk, M > 128: slices on the persistent kernel (K % 32 == 0), the generic aligned kernel
# (K % 4 == 0) and the scalar kernel (odd K); 2 slices, the 8-slice cap, a count cut by K / s >= 128; last slice full and short
SPLITK_K = {'splitk_fast': (256, 288, 320, 640, 1024, 1056), 'splitk_aligned': (260, 644, 1060), 'splitk_scalar': (257, 641, 1057)}
SPLITK_MN = ((129, 129), (257, 127), (300, 200))
_n = 0
for _route, _ks in SPLITK_K.items():
    for _K in _ks:
        for _M, _N in SPLITK_MN:
            _add('splitk', 'nt', 'splitk', _route, M=_M, N=_N, K=_K, bias=_n % 2, act=_n % 6, ldc=_N + (3 if _n % 4 == 3 else 0))
            _n += 1
_add('splitk', 'nt', 'splitk', 'splitk_scalar', M=257, N=129, K=1056, a_off=1, bias=1)
_add('splitk', 'nt', 'splitk', 'splitk_fast', M=129, N=8000, K=256, bias=1, act=1)               # 2 x 63 = 126 tiles, the most that are sliced
_add('splitk', 'nt', 'splitk', 'plain_fast', M=1930, N=1000, K=256, bias=1, act=1)              # 16 x 8 = 128 tiles: not sliced
_add('splitk', 'nt', 'splitk', 'plain_fast', M=129, N=129, K=224, bias=1)                       # K < 256: not sliced
_seam('splitk', ns=(1, 2, 5, 7, 8), last_full=(0, 1), bias=(0, 1), act=range(6))

# ---------------------------------------------------------------------------------------------------------------------
# skinny kernel: direct (algo "skinny": 16-column strips, one slice) and K slices through itr_gemm_nt_splitk with M <= 128
SKINNY_M = (1, 15, 16, 17, 64, 65, 80, 127, 128)
SKINNY_K = (128, 132, 192, 196, 256, 260, 1028)
SKINNY_N_DIRECT = (64, 65, 1000)             # (gemm_nt_algo sends fewer than 64 columns to the tile kernel; wider strips exist only sliced)
SKINNY_N_SLICED = (16, 17, 63, 64, 65, 1000, 1024, 1040, 4104)
_n = 0
for _N in SKINNY_N_DIRECT:
    for _K in SKINNY_K:
        for _M in (SKINNY_M if (_N, _K) in ((64, 128), (65, 260)) else (SKINNY_M[_n % 9], SKINNY_M[(_n + 4) % 9])):
            _add('skinny_direct', 'nt', 'algo', 'skinny_direct', M=_M, N=_N, K=_K, algo='skinny', bias=_n % 2, act=_n % 6,
                 ldc=_N + (2 if _n % 3 == 2 else 0))
            _n += 1
_seam('skinny_direct', M=SKINNY_M, N=SKINNY_N_DIRECT, K=SKINNY_K, row_tiles=(1, 2, 4, 5, 8))
for _N in SKINNY_N_SLICED:
    _w = 64 if _N >= 4096 else (32 if _N >= 1024 else 16)
    for _K in SKINNY_K:
        for _M in (SKINNY_M if (_N, _K) in ((17, 260), (1040, 1028)) else (SKINNY_M[_n % 9], SKINNY_M[(_n + 4) % 9])):
            _add('skinny_sliced', 'nt', 'splitk', 'skinny_sliced%d' % _w, M=_M, N=_N, K=_K, bias=_n % 2, act=_n % 6,
                 ldc=_N + (2 if _n % 3 == 2 else 0))
            _n += 1
for _M in (80, 128):
    _add('skinny_sliced', 'nt', 'splitk', 'skinny_sliced64', M=_M, N=2048, K=4096, bias=1)          # the other 64-column condition
_seam('skinny_sliced', M=SKINNY_M, N=SKINNY_N_SLICED + (2048,), K=SKINNY_K + (4096,), last_full=(0, 1),
      route=('skinny_sliced16', 'skinny_sliced32', 'skinny_sliced64'))

# ---------------------------------------------------------------------------------------------------------------------
# TN: three tile sizes with ragged edges, aligned / scalar, R below and above one 16-row chunk, slice counts on both sides of the
# reduce kernel's 16-way unrolled sum (a short last slice), accumulate, column sums, ldc > Q
TN_PQ = ((1, 1), (31, 40), (40, 31), (32, 32), (33, 64), (64, 200), (65, 65), (129, 132), (132, 136), (300, 129), (36, 1028))
TN_MIN = (1, 31, 32, 33, 64, 65, 129)
TN_R = (0, 1, 15, 16, 17)
TN_NSL = (1, 2, 15, 16, 17, 33)
_n = 0
for _P, _Q in TN_PQ:
    for _R in TN_R + tuple(tn_rows_for(_s, _P, _Q) for _s in TN_NSL[1:]):
        _al = tn_aligned(_P, _Q, _P, _Q)
        _add('tn', 'tn', 'tn', 'tn%d_%s' % (tn_tile(_P, _Q), 'aligned' if _al else 'scalar'), R=_R, P=_P, Q=_Q, acc=int(_n % 3 == 1),
             colsum=int(_n % 2 == 0), ldc=_Q + (4 if _n % 5 == 2 else 0))
        _n += 1
for _P, _Q in ((32, 64), (132, 68)):                    # aligned widths behind a 4-byte offset, or in rows of odd length: scalar
    for _R in (17, tn_rows_for(2, _P, _Q)):
        _add('tn', 'tn', 'tn', 'tn%d_scalar' % tn_tile(_P, _Q), R=_R, P=_P, Q=_Q, a_off=1, lda=_P + 4, colsum=1)
        _add('tn', 'tn', 'tn', 'tn%d_scalar' % tn_tile(_P, _Q), R=_R, P=_P, Q=_Q, ldb=_Q + 1, acc=1)
        _add('tn', 'tn', 'tn', 'tn%d_aligned' % tn_tile(_P, _Q), R=_R, P=_P, Q=_Q, a_off=4, b_off=8, lda=_P + 8, ldb=_Q + 12, colsum=1)
_seam('tn', minPQ=TN_MIN, R=TN_R, nsl=TN_NSL, acc=(0, 1), colsum=(0, 1), T=(32, 64, 128), a_off=(0, 1, 4))

TNB = ((0, 5, 7), (1, 1, 1), (15, 31, 33), (16, 32, 32), (17, 64, 36), (14, 9, 11), (257, 16, 17), (3, 65, 65), (36, 129, 132), (20, 132, 136))
for _R, _P, _Q in TNB:
    for _Bn in (1, 3):
        _add('tn_batched', 'tn_batched', 'tn_batched', 'tnb%d_%s' % (tn_tile(_P, _Q), 'aligned' if tn_aligned(_P, _Q, _P, _Q, 0, 0, _R * _P, _R * _Q)
                                                                     else 'scalar'), batch=_Bn, R=_R, P=_P, Q=_Q)
for _Bn in (1, 3):
    _add('tn_batched', 'tn_batched', 'tn_batched', 'tnb32_scalar', batch=_Bn, R=16, P=32, Q=32, pad_a=1)     # batch stride % 4 != 0
    _add('tn_batched', 'tn_batched', 'tn_batched', 'tnb128_scalar', batch=_Bn, R=36, P=129, Q=132, pad_b=2)
    _add('tn_batched', 'tn_batched', 'tn_batched', 'tnb32_aligned', batch=_Bn, R=16, P=32, Q=32, pad_a=4, pad_b=8)
_seam('tn_batched', batch=(1, 3), R=(0, 1, 15, 16, 17), T=(32, 64, 128), pad_a=(0, 1))

GROUPS = sorted(set(c.group for c in CASES))
