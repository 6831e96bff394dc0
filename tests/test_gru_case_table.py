"""No GPU: the case table of the GRU sweep (tests/helpers/gru_cases.py) is fit for its purpose.

Coverage: every seam value of the launch code (D, E, lengths and prefixes, token kinds, both directions) keeps a case, every route of
the per-step recurrence product is reached by a uni- and by a bi-GRU, forward and backward, and one batch changes route between two
consecutive steps in each pass; taking the sole carrier of any of these out of the table is noticed.  Tolerance: every compared
tensor's bound is at most 2^-12 of its largest value.  Sensitivity: each claimed defect moves a compared tensor by at least 10 x the
bound the GPU sweep applies.  Pins: the constants and gates the mirrors copy are checked against the source text of csrc/, so an edit
to the planning fails here instead of silently moving the seams."""
import os
import re
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gru_cases as G               # noqa: E402
import gemm_cases as GC             # noqa: E402
import train_prim_cases as P        # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-text-retrieval_amd", "csrc")

# what the table must hold, stated here a second time: an edit that shrinks SEAMS in the helper does not shrink the requirement
REQUIRED = {
    'D': (1, 32, 36, 84, 85, 86, 255, 256, 257, 258, 260, 340, 344, 1020, 1024, 1364, 1368),
    'E': (1, 5, 127, 128, 129, 300),
    'tokens': ('random', 'repeated', 'dense'),
    'bi': (0, 1),
    'lengths': ('B=1', 'all lengths 1', 'all lengths equal', 'one long caption, the others of length 1', 'never leaves the tile kernel'),
    'prefix': (130, 129, 128, 2, 65, 64, 17, 16, 15, 257, 1),
    'prefix@D256': (130, 129, 128, 2),
    'B': (1, 257),
    'eval_projection': ('vocabulary_table', 'per_token'),
    'fwd_route': ('direct_fast', 'direct_aligned', 'direct_scalar', 'tile_scalar', 'tile_aligned', 'skinny16', 'skinny32', 'skinny64'),
    'bwd_route': ('direct_fast', 'direct_aligned', 'direct_scalar', 'tile_scalar', 'tile_aligned', 'skinny16', 'skinny32'),
}
REQUIRED['fwd_route@bi'] = tuple((r, b) for r in REQUIRED['fwd_route'] for b in (0, 1))
REQUIRED['bwd_route@bi'] = tuple((r, b) for r in REQUIRED['bwd_route'] for b in (0, 1))


def missing(cases, seams):
    """[(parameter, value)] of `seams` that no case of `cases` carries, plus the two route-change requirements."""
    seen = {}
    for c in cases:
        for k, vs in c.seams().items():
            seen.setdefault(k, set()).update(str(v) for v in vs)
    out = [(k, v) for k, vs in seams.items() for v in vs if str(v) not in seen.get(k, ())]
    out += [('route change', w) for w in ('fwd', 'bwd') if not any(c.route_changes(w) for c in cases)]
    return out


def test_every_seam_value_and_every_route_has_a_case():
    assert not missing(G.CASES, G.SEAMS), missing(G.CASES, G.SEAMS)
    assert not missing(G.CASES, REQUIRED), missing(G.CASES, REQUIRED)
    for k, vs in REQUIRED.items():
        assert set(str(v) for v in vs) <= set(str(v) for v in G.SEAMS[k]), k
    assert G.FWD_ROUTES == REQUIRED['fwd_route'] and G.BWD_ROUTES == REQUIRED['bwd_route']
    assert len(G.CASES) <= 48 and len(set(c.name for c in G.CASES)) == len(G.CASES)


def test_taking_out_a_sole_carrier_is_noticed():
    """The mutation check: for every required value carried by exactly one case, the table without that case fails the coverage."""
    sole = {}
    for k, vs in REQUIRED.items():
        for v in vs:
            carriers = [c for c in G.CASES if str(v) in set(str(s) for s in c.seams().get(k, ()))]
            if len(carriers) == 1:
                sole.setdefault(carriers[0].name, []).append((k, v))
    for w in ('fwd', 'bwd'):
        carriers = [c for c in G.CASES if c.route_changes(w)]
        if len(carriers) == 1:
            sole.setdefault(carriers[0].name, []).append(('route change', w))
    assert len(sole) >= 4, sole            # (D = 1020 and 1364, the uni and the bi carrier of the 64-column strips, ...)
    for name, what in sole.items():
        rest = [c for c in G.CASES if c.name != name]
        assert set(what) <= set(missing(rest, REQUIRED)), (name, what)


def test_table_shapes_follow_the_rules():
    for c in G.CASES:
        assert list(c.lens) == sorted(c.lens, reverse=True) and c.lens[-1] >= 1 and c.n_tok == sum(c.lens), c
        assert c.prefix[0] == c.B and len(c.prefix) == c.Lmax, c
        if c.D >= 1020:
            assert c.B <= 5 and c.Lmax <= 4, c
        x = c.inputs()
        assert x['tokens'].dtype == torch.int64 and int(x['tokens'].min()) >= 0 and int(x['tokens'].max()) < c.V, c
        if c.tokens == 'random':
            assert c.V > c.n_tok, c
        elif c.tokens == 'repeated':
            assert c.V == 3, c
        else:
            assert c.V == c.n_tok and sorted(x['tokens'].tolist()) == list(range(c.n_tok)), c
        assert c.eval_projection == ('vocabulary_table' if 2 * c.V <= c.n_tok else 'per_token')
        assert x['embed'].shape == (c.V, c.E) and x['g_out'].shape == (c.n_tok, c.D)
        assert x['weight_ih_l0'].shape == (3 * c.D, c.E) and x['weight_hh_l0'].shape == (3 * c.D, c.D) and x['bias_hh_l0'].shape == (3 * c.D,)
        assert ('weight_hh_l0_reverse' in x) == c.bi
        # the reference's initial scales
        assert c.scale == 1.0 and float(x['embed'].abs().max()) <= 0.1 and float(x['weight_hh_l0'].abs().max()) <= c.D ** -0.5 * (1 + 1e-6)
    # the two hand-over batches: tile partials -> skinny partials between consecutive steps, forward and backward
    for c in G.CASES:
        if c.prefix == [130, 129, 128, 2]:
            assert [s[2] for s in c.steps['fwd']] == ['tile_aligned', 'tile_aligned', 'skinny16', 'skinny16'], c
            assert [s[2] for s in c.steps['bwd']] == ['skinny16', 'skinny16', 'tile_aligned'], c
            assert [s[3] for s in c.steps['fwd']] == [2, 2, 2, 2] and [s[3] for s in c.steps['bwd']] == [6, 6, 6], c
    assert sum(1 for c in G.CASES if c.prefix == [130, 129, 128, 2]) == 2


def test_planning_mirrors():
    sk = G.splitk_choice
    # K < 256 keeps one slice; D = 85 | 86 (backward, K = 3D) and 255 | 256 (forward, K = D)
    assert [sk(4, 3 * D, D) for D in (1, 32, 85, 86, 255, 256, 257, 1024, 1368)] == [1, 1, 1, 1, 1, 2, 2, 8, 7]
    assert [sk(4, D, 3 * D) for D in (1, 32, 85, 86, 255, 256, 257, 1024, 1368)] == [1, 1, 1, 2, 5, 6, 6, 16, 16]
    assert sk(257, 768, 256) == 2 and sk(257, 256, 768) == 6 and sk(130, 768, 256) == 2
    assert sk(128 * 128, 128, 4096) == 1 and sk(128, 128 * 127, 4096) == 2         # 128 tiles are not sliced, 127 are
    pr = G.product_route
    assert pr(1, 4, 96, 32) == ('direct_fast', 1, 32) and pr(1, 4, 255, 85) == ('direct_scalar', 1, 85) and pr(1, 4, 108, 36)[0] == 'direct_aligned'
    assert pr(2, 4, 768, 256) == ('skinny16', 2, 128) and pr(2, 128, 768, 256)[0] == 'skinny16' and pr(2, 129, 768, 256) == ('tile_aligned', 2, 128)
    assert pr(2, 4, 771, 257) == ('tile_scalar', 2, 160) and pr(2, 4, 774, 258)[0] == 'tile_scalar' and pr(2, 4, 86, 258) == ('tile_scalar', 2, 160)
    assert pr(2, 4, 1020, 340)[0] == 'skinny16' and pr(2, 4, 1032, 344)[0] == 'skinny32'
    assert pr(7, 4, 4092, 1364)[0] == 'skinny32' and pr(7, 4, 4104, 1368) == ('skinny64', 8, 192)
    assert pr(16, 4, 1020, 3060)[0] == 'skinny16' and pr(16, 4, 1024, 3072)[0] == 'skinny32' and pr(16, 4, 1368, 4104)[0] == 'skinny32'
    assert G.prefixes((4, 3, 3, 1)) == [4, 3, 3, 1] and G.prefixes((1, 1, 1)) == [3] and G.prefixes((3,)) == [1, 1, 1]
    c = next(c for c in G.CASES if c.D == 86 and c.lens == (4, 3, 3, 1) and not c.bi)
    assert [s[:4] for s in c.steps['fwd']] == [(0, 4, 'direct_scalar', 1), (1, 3, 'direct_scalar', 1), (2, 3, 'direct_scalar', 1), (3, 1, 'direct_scalar', 1)]
    assert [s[:4] for s in c.steps['bwd']] == [(3, 1, 'tile_scalar', 2), (2, 3, 'tile_scalar', 2), (1, 3, 'tile_scalar', 2)]
    assert c.grow_steps == [1, 3] and c.claims == ('a', 'bb', 'c', 'd', 'e')


def test_tolerance_is_tight():
    for c in G.CASES:
        ref = c.reference()
        assert set(ref) == set(c.tensors) | {'last'}, c
        assert ref['out'][0].shape == (c.n_tok, c.D) and ref['last'][0].shape == (c.B, c.D) and ref['d_embed'][0].shape == (c.V, c.E), c
        for name, (want, e32, e_mirror, tol) in ref.items():
            m = float(want.abs().max())
            assert bool(torch.isfinite(want).all()) and e32 == e32, (c, name)
            assert (e_mirror is not None) == (c.name in G.FALLBACK), (c, name)
            assert tol == G.FACTOR * max(e32, e_mirror or 0.0, G.U * m), (c, name)
            assert tol <= G.CAP * m, "%s %s: tol %.3g is %.3g of max|want| %.3g" % (c, name, tol, tol / m if m else 0, m)
            # a tensor that is zero in exact arithmetic: only W_hh's gradient of a batch whose every state starts from h = 0
            assert m > 0 or (c.Lmax == 1 and name.startswith('d_weight_hh')), (c, name)


def test_bound_sees_every_claimed_defect():
    claimed = {}
    for c in G.CASES:
        split_f = any(s[3] > 1 for s in c.steps['fwd'][1:])
        split_b = any(s[3] > 1 for s in c.steps['bwd'])
        grows = c.Lmax > 1 and len(set(c.prefix)) > 1
        want_claims = sorted(['c', 'e'] + (['a'] if c.Lmax > 1 else []) + (['bf'] if split_f else []) + (['bb'] if split_b else []) +
                             (['d'] if grows else []) + (['f'] if c.bi else []))
        assert list(c.claims) == want_claims, c
        ref = c.reference()
        for letter, value in c.defects().items():
            moved = max((float((value[k] - ref[k][0]).abs().max()) / ref[k][3]) if ref[k][3] > 0 else 0.0 for k in c.tensors)
            assert moved >= G.SENSITIVITY, "%s defect %s moves no tensor by more than %.3g x its bound" % (c, letter, moved)
            claimed.setdefault(letter, []).append(c)
    assert set(claimed) == set(G.DEFECTS)
    # every sliced route is claimed by the slice defect of its pass
    assert set(r for c in claimed['bf'] for r in c.fwd_routes) >= {'tile_scalar', 'tile_aligned', 'skinny16', 'skinny32', 'skinny64'}
    assert set(r for c in claimed['bb'] for r in c.bwd_routes) >= {'tile_scalar', 'tile_aligned', 'skinny16', 'skinny32'}
    assert any(c.route_changes('bwd') for c in claimed['d'])


def test_sliced_mirror_is_the_references_function():
    """The fallback's mirror (the recurrence products summed in the kernels' slices) in float64 is the reference."""
    for c in G.CASES:
        if c.group != 'prefix' and not (c.D in (86, 257, 1368) and not c.bi):
            continue
        ref, m64 = c.reference(), c.evaluate(torch.float64, sliced=True)
        for k in c.tensors:
            assert float((m64[k] - ref[k][0]).abs().max()) <= 1e-11 * max(1.0, float(ref[k][0].abs().max())), (c, k)


def test_fallback_list_and_constants():
    assert G.FALLBACK <= set(c.name for c in G.CASES)
    assert G.FACTOR == P.FACTOR == 16 and G.U == P.U == 2.0 ** -24 and G.SENSITIVITY == P.SENSITIVITY == 10 and G.CAP == 2.0 ** -12
    assert G.skinny_ok is GC.skinny_ok and G.skinny_plan is GC.skinny_plan and G.nt_kernel is GC.nt_kernel


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_constants_are_the_ones_of_the_source():
    """The mirrors' constants and gates, as the source text states them (whitespace folded)."""
    text = {n: _src(n) for n in ("gemm_f32.hip", "gemm_skinny.hip", "gru_train.hip", "towers.hip")}
    assert "constexpr int BM = %d, BN = %d, BK = %d," % (GC.BM, GC.BN, GC.BK) in text["gemm_f32.hip"]
    assert "constexpr int SK_KC = %d, SK_MAXM = %d;" % (GC.SK_KC, GC.SK_MAXM) in text["gemm_skinny.hip"]
    pins = {
        "gemm_f32.hip": (
            # gemm_splitk_choice
            "int gemm_splitk_choice(int64_t M, int64_t N, int64_t K) { const int64_t tiles = ceil_div(M, BM) * ceil_div(N, BN); "
            "if (tiles >= 128 || K < %d) return 1; int s_ = (int)(%d / tiles); while (s_ > 1 && K / s_ < %d) --s_; "
            "return s_ < 1 ? 1 : (s_ > %d ? %d : s_); }" % (G.SPLITK_MIN_K, G.SPLITK_TARGET, G.SPLITK_MIN_SLICE, G.SPLITK_MAX, G.SPLITK_MAX),
            # gemm_nt_splitk with one slice: the tile kernel directly
            "if (splits <= 1) { GemmArgs g1{A, B, bias, C, lda, ldb, ldc, M, N, K, act, 1, BM, nullptr, nullptr, 0, accumulate, 0, nullptr}; "
            "return launch_gemm(g1, st); }",
            # gemm_nt_splitk_partials
            "if (splits > 1 && fit >= 1 && gemm_skinny_ok(A, lda, B, ldb, M, N, K))",
            "return gemm_skinny_partials(A, lda, B, ldb, M, N, K, fit < %d ? (int)fit : %d, scratch, n_slices, st);" % ((G.PARTIALS_MAX_SLICES,) * 2),
            "const int64_t ksplit = ceil_div(ceil_div(K, (int64_t)(splits > 1 ? splits : 1)), (int64_t)BK) * BK; const int ns = (int)ceil_div(K, ksplit); "
            "ITR_REQUIRE((size_t)ns <= fit,",
            "GemmArgs g{A, B, nullptr, scratch, lda, ldb, N, M, N, K, 0, 1, BM, nullptr, nullptr, 0, 0, ksplit, scratch};",
            # launch_gemm's choice of loader
            "const bool fast = aligned && g.group <= 1 && (g.K % BK == 0) && g.K >= BK && g.rows_per_tile == BM &&",
        ),
        "gemm_skinny.hip": (
            "return M >= 1 && M <= SK_MAXM && N >= 16 && K >= SK_KC && K % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 &&",
            "const int nc = (N >= 4096 || (N >= 2048 && K >= 4096)) ? 4 : (N >= 1024 ? 2 : 1);",
            "if (s > max_slices) s = max_slices;",
        ),
        "gru_train.hip": (
            "t.sk_bytes = gemm_splitk_scratch_bytes(B, 3 * D, %d);" % G.PARTIALS_MAX_SLICES,
            # the forward's plan and its per-step call
            "const int splits_h = gemm_splitk_choice(B, 3 * D, D);",
            "while (n_act > 0 && len_host[n_act - 1] <= t) --n_act;",
            "if (splits_h > 1) rc2 = gemm_nt_splitk_partials(d.h, D, wh, D, n_act, 3 * D, D, splits_h, d.skbuf, w.sk_bytes, &ns, sd);",
            "else rc2 = gemm_nt_splitk(d.h, D, wh, D, bh, d.gh, 3 * D, n_act, 3 * D, D, 0, 0, splits_h, d.skbuf, sd);",
            # the backward's
            "const int splits_c = gemm_splitk_choice(B, D, 3 * D);",
            "while (n_act < B && len_host[n_act] > t) ++n_act;",
            "GB_TRY(gemm_nt_splitk_partials(d.dgh_step, 3 * D, d.whhT, 3 * D, n_act, D, 3 * D, splits_c, d.skbuf, w.sk_bytes, &ns_pending, sd)); prev_n = n_act;",
            "GB_TRY(gemm_nt_splitk(d.dgh_step, 3 * D, d.whhT, 3 * D, nullptr, d.carry, D, n_act, D, 3 * D, 0, 1, splits_c, d.skbuf, sd));",
            # the consumers of the slices
            "for (int s_ = 1; s_ < ns; ++s_) { g0 += ghr[s_ * ss + j];",
            "if (ns > 0 && b < prev_n) {",
            "for (int s_ = 0; s_ < ns; ++s_) cin += part[s_ * ss + b * D + j];",
            # block edges
            "dim3((unsigned)n_act, (unsigned)ceil_div(D, %d)), dim3(%d), 0, sd, d.gi," % (G.GATE_BLOCK, G.GATE_BLOCK),
            "dim3((unsigned)n_act, (unsigned)ceil_div(D, %d)), dim3(%d), 0, sd, d_out," % (G.GATE_BLOCK, G.GATE_BLOCK),
            "__shared__ float t[%d][%d];" % (G.TRANSPOSE_TILE, G.TRANSPOSE_TILE + 1),
            "dim3((unsigned)ceil_div(cols, %d), (unsigned)ceil_div(ldo, %d)), dim3(256)," % (G.TRANSPOSE_TILE, G.TRANSPOSE_TILE),
            "hipLaunchKernelGGL(embed_gather_train_kernel, dim3((unsigned)n_tok), dim3(%d), 0, st, tokens," % G.GATHER_THREADS,
            "hipLaunchKernelGGL(gru_avg_kernel, dim3((unsigned)ceil_div(n, (int64_t)256)), dim3(256),",
        ),
        "towers.hip": (
            "const bool table = 2 * V <= n_tok && !want_per_token;",
            "const int splits_h = (B <= 1024 && !batch_invariant) ? gemm_splitk_choice(B, 3 * D, D) : 1;",
        ),
    }
    for name, lines in pins.items():
        for line in lines:
            assert line in text[name], "%s no longer says: %s" % (name, line)
    assert text["gru_train.hip"].count("gemm_splitk_choice(") == 2 and text["gru_train.hip"].count("gemm_nt_splitk_partials(") == 2
