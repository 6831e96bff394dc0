"""No GPU: the case table of the evaluation-tower sweep (tests/helpers/tower_cases.py) is fit for its purpose.

Coverage: every seam value of the launch code keeps a case -- every (attention route, NT, dk), pair counts below, at and one above the
waves per workgroup of every (route, NT), both chunk counts, both passes of the gate's persistent loop, both norm routes for every
kind -- and taking the sole carrier of any of these out of the table is noticed.  Routes: the mirrors put each case on the route it is
listed under.  Tolerance: every compared tensor's bound is at most 2^-12 of its largest value.  Sensitivity: each named defect moves a
compared tensor by at least 10 x the bound the GPU sweep applies.  Pins: the constants the mirrors copy are checked against the source
text of csrc/ and of ops.py, so an edit to the dispatch fails here instead of silently moving the seams."""
import os
import re
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import tower_cases as T             # noqa: E402
import train_prim_cases as P        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "image-text-retrieval_amd", "csrc")

# what the table must hold, stated here a second time: an edit that shrinks SEAMS in the helper does not shrink the requirement
_MHA_DK = (16, 32, 64)
_ACTS = ('none', 'relu', 'tanh', 'sigmoid', 'gelu', 'leaky_relu')
REQUIRED = {
    'attention.L': (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64),
    'attention.dk': _MHA_DK,
    'attention.mask': (0, 1),
    'attention.layout': ('fused', 'camera', 'fused+1', 'stride3A+1'),
    'attention.pairs': (1, 3, 4, 5, 9),
    'attention.mask_kind': ('ragged', 'holes'),
    'attention.last_key': ('kept', 'masked'),
    'attention.route_nt_dk': tuple((r, nt, dk) for r in ('reg', 'lds') for nt in (1, 2, 3, 4) for dk in _MHA_DK) + tuple(('valu', 0, dk) for dk in _MHA_DK),
    'attention.route_nt_count': tuple((r, nt, c) for r in ('reg', 'lds') for nt in (1, 2, 3, 4) for c in ('below', 'equal', 'above')) +
                                (('valu', 0, 'equal'), ('valu', 0, 'above')),
    'add_layernorm.rows': (1, 3, 4, 5, 9), 'add_layernorm.H': (4, 252, 256, 260, 768, 4096), 'add_layernorm.res': (0, 1),
    'bert_embed_ln.rows': (1, 3, 4, 5, 9), 'bert_embed_ln.H': (4, 252, 256, 260, 768, 4096), 'bert_embed_ln.types': (0, 1),
    'bert_embed_ln.L_vs_max_pos': ('below', 'equal'),
    'relu_maxpool.C': (1, 255, 256, 257), 'relu_maxpool.valid': ('1', 'L-1', 'L'), 'relu_maxpool.chunks': (1, 2),
    'mean_mid.F': (1, 3, 4, 5, 1023, 1024, 1028), 'mean_mid.R': (1, 36), 'mean_mid.chunks': (1, 2), 'mean_mid.chunks_F': ((2, 4), (2, 5)),
    'agsa_gate.dk': (16, 32), 'agsa_gate.rows': (1, 15, 16, 17, 63, 64, 65, 131072, 131093),
    'agsa_gate.passes_dk': ((1, 16), (1, 32), (2, 16), (2, 32)),
    'gcn_relation.N': (1, 2, 3, 35, 36), 'gcn_relation.D': (4, 60, 64, 68, 260, 2048), 'gcn_relation.n_img': (1, 3), 'gcn_relation.ld': ('3D', '3D+4'),
    'camera_summarize.R': (1, 36, 63, 64), 'camera_summarize.k': (1, 12), 'camera_summarize.D': (1, 255, 256, 257, 2048),
    'camera_posenc.boxes': (1, 255, 256, 257),
    'affine_cols.act_scale_res': tuple((a, s, r) for a in _ACTS for s in (0, 1) for r in (0, 1)),
    'affine_cols.n': (1, 255, 256, 257), 'affine_cols.C': (1, 3, 257),
    'mul_rows.n': (255, 256, 257),
    'norm.kind_abs': tuple((k, a) for k in (0, 1, 2, 3) for a in (0, 1)), 'norm.dim': (1, 3, 4, 252, 256, 260, 4096, 4100), 'norm.rows': (1, 3, 4, 5),
    'norm.route_kind': tuple((r, k) for r in ('vec', 'scalar') for k in (0, 1, 2, 3)),
    'norm.route_dim': (('vec', 'dim%4==0'), ('scalar', 'dim%4==0'), ('scalar', 'other')),
    'norm.special_rows': tuple((k, 'small and zero row') for k in (0, 1, 2, 3)),
}

# the defects every family must claim somewhere (the issue's table)
REQUIRED_DEFECTS = {
    'attention': ('last key dropped', 'padding key counted', 'mask ignored', 'neighbour head'),
    'add_layernorm': ('last float4 out of the mean', 'residual dropped'),
    'bert_embed_ln': ('last float4 out of the mean', 'position t - 1', 'type embedding ignored'),
    'relu_maxpool': ('valid one too small', 'valid one too large', 'second chunk lost'),
    'mean_mid': ('last group lost', 'second chunk lost'),
    'agsa_gate': ('gate halves swapped', 'second-pass tile unwritten'),
    'gcn_relation': ('partial last chunk dropped', 'region N - 1 dropped', 'divisor 36'),
    'camera_summarize': ('last region dropped', 'norm over the first 256 columns'),
    'camera_posenc': ('last box unwritten',),
    'affine_cols': ('activation after the residual', 'last element unwritten'),
    'mul_rows': ('ldb ignored',),
    'norm': ('eps inside the sqrt', 'l1 and l2 exchanged'),
}


def missing(cases, seams):
    """[(parameter, value)] of `seams` that no case of `cases` carries."""
    seen = {}
    for c in cases:
        for k, vs in c.seams().items():
            seen.setdefault(k, set()).update(str(v) for v in vs)
    return [(k, v) for k, vs in seams.items() for v in vs if str(v) not in seen.get(k, ())]


def test_every_seam_value_and_every_route_has_a_case():
    assert not missing(T.CASES, T.SEAMS), missing(T.CASES, T.SEAMS)
    assert not missing(T.CASES, REQUIRED), missing(T.CASES, REQUIRED)
    for k, vs in REQUIRED.items():
        assert set(str(v) for v in vs) <= set(str(v) for v in T.SEAMS[k]), k
    assert set(c.family for c in T.CASES) == set(T.FAMILIES) == set(REQUIRED_DEFECTS)
    assert len(set(c.name for c in T.CASES)) == len(T.CASES) and T.ACTS == _ACTS and T.MHA_DKS == _MHA_DK
    # every attention case exists without and with a mask
    att = T.cases('attention')
    assert sorted(c.name.replace('-mask1', '-mask0') for c in att if c.shape['mask']) == sorted(c.name for c in att if not c.shape['mask'])


def test_taking_out_a_sole_carrier_is_noticed():
    """The mutation check: for every required value carried by exactly one case, the table without that case fails the coverage."""
    sole = {}
    for k, vs in REQUIRED.items():
        for v in vs:
            carriers = [c for c in T.CASES if str(v) in set(str(s) for s in c.seams().get(k, ()))]
            assert carriers, (k, v)
            if len(carriers) == 1:
                sole.setdefault(carriers[0].name, []).append((k, v))
    # (the two-chunk cases, the 3D + 4 stride, the single posenc and mul_rows sizes, ...)
    assert len(sole) >= 8, sole
    assert any(('mean_mid.chunks_F', (2, 5)) in what for what in sole.values())
    for name, what in sole.items():
        rest = [c for c in T.CASES if c.name != name]
        assert set(what) <= set(missing(rest, REQUIRED)), (name, what)


def test_mirrors_put_every_case_on_its_route():
    for c in T.cases('attention'):
        e = c.extra
        A = e['heads'] * e['dk']
        route = T.mha_case_route(e['layout'], e['out'], A, e['L'])
        assert c.route == route and c.shape['route'] == route[0], c
        assert route[0] == {'fused': 'lds' if e['out'] == 'block+1' else 'reg', 'camera': 'lds' if e['out'] == 'block+1' else 'reg',
                            'fused+1': 'valu', 'stride3A+1': 'valu'}[e['layout']], c
        assert route[1] == (0 if route[0] == 'valu' else -(-e['L'] // 16)), c
        x = c.inputs()
        assert x['q'].shape == (e['B'] * e['L'], A) and bool((x['v'].view(e['B'], e['L'], A)[:, -1] >= 2.0).all()), c
        if 'mask' in x:
            assert x['mask'].shape == (e['B'], e['L']) and bool((x['mask'].sum(1) >= 1).all()) and set(x['mask'].unique().tolist()) <= {0.0, 1.0}, c
    mr = T.mha_route
    assert mr(0, 64, 128, 192, 192, 192, 0, 64, 33) == ('reg', 3, 4) and mr(0, 64, 128, 192, 192, 192, 1, 66, 33) == ('lds', 3, 2)
    assert mr(0, 64, 128, 192, 192, 192, 0, 66, 32) == ('lds', 2, 4) and mr(0, 64, 128, 192, 192, 192, 4, 68, 64) == ('reg', 4, 4)
    assert mr(1, 65, 129, 192, 192, 192, 0, 64, 16) == ('valu', 0, 1) and mr(0, 64, 128, 193, 193, 193, 0, 64, 16) == ('valu', 0, 1)
    assert mr(0, 0, 64, 64, 64, 128, 0, 64, 1) == ('reg', 1, 4) and mr(0, 0, 2, 64, 64, 128, 0, 64, 1) == ('valu', 0, 1)
    assert [T.norm_route(d, True) for d in (1, 3, 4, 4096, 4100)] == ['scalar', 'scalar', 'vec', 'vec', 'scalar'] and T.norm_route(256, False) == 'scalar'
    for c in T.cases('norm'):
        assert c.route == T.norm_route(c.shape['dim'], c.extra['lead'] % 4 == 0), c
    assert [T.agsa_passes(r) for r in (1, 64, 65, 131072, 131073, 131093, 262144, 262145)] == [1, 1, 1, 1, 2, 2, 2, 3]
    for c in T.cases('agsa_gate'):
        assert c.route == T.agsa_passes(c.shape['rows']) == (2 if c.shape['rows'] > 131072 else 1), c
    assert [T.chunks(b) for b in (1, 65535, 65536, 131070, 131071)] == [1, 1, 2, 2, 3]
    assert sorted(c.shape['B'] for c in T.CASES if c.family in ('relu_maxpool', 'mean_mid') and T.chunks(c.shape['B']) == 2) == [65536] * 3


def test_inputs_follow_the_rules():
    for c in T.cases('add_layernorm', 'bert_embed_ln'):
        want = c.reference()['y'][0]
        assert float(want.std(-1).min()) > 0.05, c                  # no constant rows
    for c in T.cases('bert_embed_ln'):
        x = c.inputs()
        assert 0 <= int(x['ids'].min()) and int(x['ids'].max()) < x['word'].shape[0] and x['ids'].shape[1] <= x['pos'].shape[0], c
    for c in T.cases('relu_maxpool'):
        x, v = c.inputs()['x'], c.extra['valid']
        live = x[:, :, 1:] if x.shape[2] > 1 else x
        assert bool((live[:, :v].max(1).values == live[:, v - 1]).all()), c
        assert v == x.shape[1] or bool((live[:, v] > live[:, :v].max(1).values).all()), c
        assert x.shape[2] == 1 or bool((x[:, :, 0] < 0).all()), c
    for c in T.cases('norm'):
        x = c.inputs()['x']
        if c.shape['rows'] > T.ZERO_ROW:
            assert bool((x[T.ZERO_ROW] == 0).all()) and 0 < float(x[T.SMALL_ROW].abs().max()) < 1e-6, c
            want = c.reference()['y'][0]
            assert bool(torch.isnan(want[T.ZERO_ROW]).all()) if c.shape['kind'] == 3 else bool((want[T.ZERO_ROW] == 0).all()), c
            assert not bool(torch.isnan(want[[r for r in range(c.shape['rows']) if r != T.ZERO_ROW]]).any()), c
    for c in T.cases('gcn_relation'):
        assert c.extra['D'] % 4 == 0 and c.extra['ld'] % 4 == 0 and c.extra['N'] <= T.GCN_MAXN, c          # what the entry point accepts
    for c in T.cases('camera_summarize'):
        assert c.shape['R'] <= T.SUMMARIZE_MAXR, c


def test_tolerance_is_tight():
    for c in T.CASES:
        for name, (want, e32, tol, rule) in c.reference().items():
            m = T.max_abs(want)
            assert e32 == e32 and e32 != float('inf') and m > 0, (c, name)
            assert rule == ('fallback' if c.name in T.FALLBACK else 'primary'), (c, name)
            primary = T.FACTOR * max(e32, T.U * m)
            assert tol == (primary if rule == 'primary' else max(primary, c.prior(c.x64())[name])), (c, name)
            assert tol <= T.CAP * m, "%s %s: tol %.3g is %.3g of max|want| %.3g" % (c, name, tol, tol / m, m)


def test_bound_sees_every_named_defect():
    claimed = {}
    for c in T.CASES:
        ref = c.reference()
        for dname, value in c.defects().items():
            assert set(value) <= set(ref), (c, dname)
            moved = max(T.max_err(value[k], ref[k][0]) / ref[k][2] for k in value)
            assert moved >= T.SENSITIVITY, "%s defect '%s' moves no tensor by more than %.3g x its bound" % (c, dname, moved)
            claimed.setdefault((c.family, dname), []).append(c)
    for fam, names in REQUIRED_DEFECTS.items():
        for n in names:
            assert (fam, n) in claimed, (fam, n)
    # the claims follow from the shapes
    for c in T.cases('attention'):
        e, named = c.extra, set(c.named)
        assert ('padding key counted' in named) == (c.route[0] != 'valu' and e['L'] % 16 != 0 and e['L'] > 1), c
        assert ('mask ignored' in named) == (bool(c.shape['mask']) and e['L'] > 1) and ('neighbour head' in named) == (e['heads'] > 1), c
        assert ('last key dropped' in named) == (not c.shape['mask'] or bool((c.inputs()['mask'][:, -1] == 1).any())), c
    att = claimed[('attention', 'padding key counted')]
    assert set((c.route[0], c.route[1]) for c in att) == set((r, nt) for r in ('reg', 'lds') for nt in (1, 2, 3, 4))
    assert all('second chunk lost' in c.named for c in T.CASES if c.family in ('relu_maxpool', 'mean_mid') and T.chunks(c.shape['B']) == 2)
    assert all(('second-pass tile unwritten' in c.named) == (c.route == 2) for c in T.cases('agsa_gate'))
    assert all(('partial last chunk dropped' in c.named) == (c.extra['D'] % T.GCN_KC != 0) for c in T.cases('gcn_relation'))
    assert all(('eps inside the sqrt' in c.named) == (c.shape['kind'] == 0 and c.shape['rows'] >= 3) for c in T.cases('norm'))


def test_fallback_list_and_constants():
    assert T.FALLBACK <= set(c.name for c in T.CASES)
    for fam in T.FAMILIES:
        n = len(T.cases(fam))
        fb = [c for c in T.cases(fam) if c.name in T.FALLBACK]
        assert 10 * len(fb) <= n, (fam, len(fb), n)                 # at most one case in ten
        assert all(c.prior is not None for c in fb), fam
    assert T.FACTOR is P.FACTOR and T.U is P.U and T.SENSITIVITY is P.SENSITIVITY and T.Case is P.Case and T.tolerance is P.tolerance
    assert T.FACTOR == 16 and T.U == 2.0 ** -24 and T.SENSITIVITY == 10 and T.CAP == 2.0 ** -12
    assert len(T.REFUSALS) == 6
    # the a-priori terms are what they say: at least the rounding of one operation on the largest value (a case that uses one still
    # has to meet the 2^-12 cap: test_tolerance_is_tight)
    for c in T.CASES:
        if c.prior is not None:
            ref = c.reference()
            for k, v in c.prior(c.x64()).items():
                assert k in ref and v >= T.U * T.max_abs(ref[k][0]), (c, k)


def _src(*path):
    with open(os.path.join(*path)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_constants_are_the_ones_of_the_source():
    """The mirrors' constants and gates, as the source text states them (whitespace folded)."""
    text = {n: _src(CSRC, n) for n in ("transformer.hip", "agsa_gate.hip", "eltwise.hip", "vsrn.hip", "norm.hip")}
    ops = _src(ROOT, "image-text-retrieval_amd", "itr_amd", "ops.py")

    def const(name, pattern):
        m = re.search(pattern, text[name])
        assert m, "%s no longer matches: %s" % (name, pattern)
        return tuple(int(g) for g in m.groups())

    assert const("transformer.hip", r"constexpr int LN_MAXV = (\d+);") == (T.LN_MAXV,)
    assert const("norm.hip", r"constexpr int NORM_WAVES = (\d+);") == (T.NORM_WAVES,)
    assert const("norm.hip", r"constexpr int NORM_MAXV = (\d+);") == (T.NORM_MAXV,)
    assert const("vsrn.hip", r"constexpr int GCN_MAXN = (\d+);") == (T.GCN_MAXN,)
    assert const("vsrn.hip", r"constexpr int GCN_KC = (\d+);") == (T.GCN_KC,)
    a, b, c, d = const("agsa_gate.hip", r"const unsigned grid = \(unsigned\)\(want < (\d+) \* (\d+) \? want : (\d+) \* (\d+)\);")
    assert a * b == c * d == T.AGSA_GRID_CAP
    assert const("eltwise.hip", r"ITR_UNSUPPORTED\(R > (\d+),") == (T.SUMMARIZE_MAXR,)
    assert const("eltwise.hip", r"for \(int d = threadIdx\.x; d < D; d \+= (\d+)\) \{ float s = 0\.f;") == (T.SUMMARIZE_THREADS,)
    # the waves-per-workgroup table of dispatch_mha_mfma and the four pairs per workgroup of the register kernel
    table = re.findall(r"if \(nt == (\d)\) return launch_mha_mfma<DK, (\d), (\d)>", text["transformer.hip"])
    last = re.search(r"return launch_mha_mfma<DK, 4, (\d)>\(q, k, v, ldq, ldk, ldv, mask, out, ldo, B, L, heads, scale, st\); \}", text["transformer.hip"])
    assert [(int(a), int(b), int(c)) for a, b, c in table] == [(nt, nt, T.MHA_LDS_WAVES[nt]) for nt in (1, 2, 3)] and int(last.group(1)) == T.MHA_LDS_WAVES[4]
    pins = {
        "transformer.hip": (
            "const int nt = (L + 15) / 16;",
            "if (ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {",
            "const dim3 grid((unsigned)ceil_div(npairs, (int64_t)%d));" % T.MHA_REG_WAVES,
            "const int64_t pair = (int64_t)blockIdx.x * %d + (threadIdx.x >> 6);" % T.MHA_REG_WAVES,
            "const bool al = (ldq % 4 == 0) && (ldk % 4 == 0) && (ldv % 4 == 0) && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | "
            "reinterpret_cast<uintptr_t>(v)) & 15) == 0;",
            "ITR_UNSUPPORTED(L > %d," % T.MHA_MAXL,
            "ITR_UNSUPPORTED(dk != 16 && dk != 32 && dk != 64,",
            # four rows per workgroup in both LayerNorm kernels, and their width limit
            "hipLaunchKernelGGL(itr::embed_ln_kernel, dim3((unsigned)itr::ceil_div(rows, %d)), dim3(256)," % T.LN_ROWS,
            "hipLaunchKernelGGL(itr::add_ln_kernel, dim3((unsigned)itr::ceil_div(rows, %d)), dim3(256)," % T.LN_ROWS,
            "ITR_UNSUPPORTED(H % 4 != 0 || H > 64 * 4 * itr::LN_MAXV, \"itr_add_layernorm:",
            "ITR_REQUIRE(B >= 0 && B <= %d && L >= 1 && C >= 1 && valid >= 1 && valid <= L && ldo >= C," % T.CHUNK,
        ),
        "agsa_gate.hip": (
            "const int64_t wave0 = (int64_t)blockIdx.x * %d + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * %d;" % (T.AGSA_WAVES, T.AGSA_WAVES),
            "const int64_t ntiles = (rows + %d) / %d; const int64_t want = (ntiles + %d) / %d;" % (T.AGSA_TILE - 1, T.AGSA_TILE, T.AGSA_WAVES - 1, T.AGSA_WAVES),
            "for (int64_t t = wave0; t < ntiles; t += nwaves) {",
            "ITR_UNSUPPORTED(dk != 16 && dk != 32,",
        ),
        "vsrn.hip": (
            "for (int k0 = 0; k0 < D; k0 += GCN_KC) {",
            "ITR_UNSUPPORTED(N > itr::GCN_MAXN,",
            "ITR_REQUIRE(ld >= 3 * (int64_t)D && ldy >= D && ld % 4 == 0 && D % 4 == 0,",
        ),
        "norm.hip": (
            "const bool vec = (dim % 4 == 0) && (dim <= 64 * 4 * NORM_MAXV) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0) && "
            "((reinterpret_cast<uintptr_t>(y) & 15) == 0);",
            "const int64_t nblk = ceil_div(rows, NORM_WAVES);",
            "ITR_REQUIRE(B <= %d, \"itr_mean_mid: at most %d groups per call\");" % (T.CHUNK, T.CHUNK),
            "if (f + 3 < F && (F & 3) == 0) {",
            # the float4 path alone needs 16-byte rows
            "ITR_REQUIRE(F % 4 != 0 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0,",
        ),
    }
    for name, lines in pins.items():
        for line in lines:
            assert line in text[name], "%s no longer says: %s" % (name, line)
    assert text["transformer.hip"].count("(int64_t)blockIdx.x * %d + (threadIdx.x >> 6)" % T.LN_ROWS) == 3          # embed_ln, add_ln, mha_reg
    assert ops.count("for b0 in range(0, B, %d): b1 = min(B, b0 + %d)" % (T.CHUNK, T.CHUNK)) == 2
    acts = dict(re.findall(r"'(\w+)': (\d)", re.search(r"_ACTS = \{(.*?)\}", ops).group(1)))
    assert [int(acts[a]) for a in T.ACTS] == [0, 1, 2, 3, 4, 5] and "ITR_REQUIRE(act >= 0 && act <= 5," in text["eltwise.hip"]
