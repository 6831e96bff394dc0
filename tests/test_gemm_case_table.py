"""No GPU: the case table of the GEMM sweep (tests/helpers/gemm_cases.py) is fit for its purpose.

Coverage: every seam value of the launch geometry keeps a case, so a later edit cannot quietly thin the table.  Routes: the mirrors
of the host-side planning put every case on the kernel it names, with the slice counts and the short last slices the seams ask for.
Sensitivity: the float64 result with the LAST index of the reduced axis left out differs from the reference by at least 10 x the
bound the GPU sweep applies to that case -- a kernel that drops one k (or one row r of a TN product) cannot pass.  Pins: the
constants and thresholds the mirrors copy are checked against the source text of csrc/, so an edit to the kernels' geometry fails
here instead of silently moving the seams."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_cases as G        # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-text-retrieval_amd", "csrc")


def _value(case, param):
    return case.shape[param] if param in case.shape else case.plan.get(param)


@pytest.mark.parametrize("group", sorted(G.SEAMS))
def test_every_seam_value_has_a_case(group):
    have = G.cases(group)
    assert have, group
    for param, values in G.SEAMS[group].items():
        seen = set(str(_value(c, param)) for c in have)
        missing = [v for v in values if str(v) not in seen]
        assert not missing, "%s: no case with %s in %s" % (group, param, missing)


def test_seam_lists_are_the_ones_of_the_launch_geometry():
    S = G.SEAMS
    assert set(G.GROUPS) == set(S)
    for kern, ks in (('fast', {32, 64, 96, 128, 160}), ('aligned', {4, 36, 100}), ('scalar', {1, 6, 37})):
        g = S['tile_' + kern]
        assert set(g['M']) == set(g['N']) == {1, 127, 128, 129, 257} and set(g['K']) == ks and set(g['bias']) == {0, 1}
        for K in ks:        # the whole M x N grid at every K
            assert len(set((c.shape['M'], c.shape['N']) for c in G.cases('tile_' + kern) if c.shape['K'] == K)) == 25
    assert set(S['tile_fast']['nk']) == {1, 2, 3, 4, 5}
    assert set(S['tile_count']['tiles']) == {1, 7, 8, 9, 529}
    assert set(S['epilogue']['act']) == set(range(7)) and set(S['strides']['K']) >= {0, 64} and set(S['strides']['a_off']) == {0, 1}
    assert set(S['groupmax']['k']) == {1, 2, 3, 12, 37, 64, 65, 128} and set(S['groupmax']['rows_per_tile']) == {128, 126, 120, 111, 65}
    assert set(S['groupmax']['Nc']) == {127, 128, 129} and set(S['groupmax']['D']) == {7, 8}
    st = S['stream']
    assert set(st['tiles_n']) == {1, 3, 4, 8} and set(st['nk2']) == {2, 3, 4, 5} and set(st['act']) == {0, 1, 4} and set(st['rest']) == {0, 5}
    for res in (512, 256):
        assert set(st['tn:tm@%d' % res]) == set('%d:%s' % (n, l) for n in (1, 3, 4, 8) for l in ('1', 'W-1', 'W', 'W+1', '2W+1'))
    assert set(S['splitk']['ns']) >= {2, 5, 8} and set(S['splitk']['last_full']) == {0, 1}
    for g in ('skinny_direct', 'skinny_sliced'):
        assert set(S[g]['M']) == {1, 15, 16, 17, 64, 65, 80, 127, 128} and set(S[g]['K']) >= {128, 132, 192, 196, 260, 1028}
    assert set(S['skinny_direct']['N']) == {64, 65, 1000}
    assert set(S['skinny_sliced']['N']) == {16, 17, 63, 64, 65, 1000, 1024, 1040, 2048, 4104}
    assert set(S['tn']['minPQ']) == {1, 31, 32, 33, 64, 65, 129} and set(S['tn']['R']) == {0, 1, 15, 16, 17}
    assert set(S['tn']['nsl']) == {1, 2, 15, 16, 17, 33} and set(S['tn_batched']['batch']) == {1, 3}


def test_the_mirrors_put_every_case_on_its_route():
    assert len(set(c.name for c in G.CASES)) == len(G.CASES)
    for c in G.CASES:
        assert c.plan['route'] == c.route, (c, c.plan)


def test_tile_kernel_cases_reach_their_seams():
    for c in G.cases('tile_fast'):
        assert c.plan['nk'] == c.shape['K'] // 32
    walks = {c.plan['tiles']: c.plan['walk'] for c in G.cases('tile_count') if c.route == 'fast'}
    assert walks[1] == (8, 1, 1) and walks[7] == (8, 1, 1)            # fewer than 8 tiles: XCD ranges of one tile and of none
    assert walks[8] == (8, 1, 1) and walks[9] == (16, 2, 1)           # ntile % 8 != 0: the first XCD walks one tile more
    assert walks[529] == (512, 67, 2)                                   # 67 tiles on 64 slots: `tt` takes a second trip
    assert set(c.plan['tiles'] for c in G.cases('tile_count') if c.route == 'aligned') == set(walks)
    # every activation code, with and without bias, on each of the three kernels; accumulate and residual on each as well
    epi = G.cases('epilogue')
    for kern in ('fast', 'aligned', 'scalar'):
        assert set((c.shape['act'], c.shape['bias']) for c in epi if c.route == kern and c.entry == 'algo') == \
            set((a, b) for a in range(6) for b in (0, 1))
        assert any(c.shape['act'] == 6 and c.entry == 'nt' and c.shape['nan'] for c in epi if c.route == kern)
        assert any(c.entry == 'acc' and c.shape['ldc'] > c.shape['N'] for c in epi if c.route == kern)
        assert any(c.entry == 'residual' and c.shape['ldr'] > c.shape['N'] for c in epi if c.route == kern)
    st = G.cases('strides')
    for kern in ('fast', 'aligned', 'scalar'):
        assert any(c.shape['lda'] > c.shape['K'] > 0 for c in st if c.route == kern)
        assert any(c.shape['lda'] < c.shape['K'] for c in st if c.route == kern)
    assert all(c.shape['ldc'] > c.shape['N'] for c in st if c.shape['K'] > 0)
    assert any(c.shape['a_off'] == 1 and c.shape['K'] == 64 and c.route == 'scalar' for c in st)
    gm = G.cases('groupmax')
    for k in G.MVM_K:       # Ni on both sides of one row tile, at every Nc and both D
        per_tile = (128 // k)
        have = set((c.shape['Ni'], c.shape['Nc'], c.shape['D']) for c in gm if c.shape['k'] == k)
        assert have >= set((ni, nc, d) for ni in (per_tile, per_tile + 1) for nc in G.MVM_NC for d in G.MVM_D), k


def test_stream_cases_reach_the_row_range_split_and_the_xcd_map():
    cs = G.cases('stream')
    for res in G.RESIDENT:
        plans = [c.plan['stream@%d' % res] for c in cs]
        for tn in G.STREAM_TN:
            mine = [p for p in plans if p['tiles_n'] == tn]
            assert any(p['idle'] > 0 for p in mine)                            # ntile == 0: workgroups that return at once
            assert any(p['q'] == 1 and p['r'] == 0 for p in mine)              # one tile each
            assert any(p['q'] >= 1 and p['r'] == 1 for p in mine)              # iw < r_ for the first workgroup only
            assert any(p['q'] >= 2 and p['r'] == 1 for p in mine)                # more than one round, and a ragged one
            assert all(p['xcd_map'] == (1 if tn >= 4 else 0) for p in mine), (res, tn)
    assert set((c.shape['K'] // 64) for c in cs) == {2, 3, 4, 5}
    assert any(c.shape['ldc'] > c.shape['N'] for c in cs) and any(c.shape['lda'] < c.shape['K'] for c in cs)
    assert set((c.shape['act'], c.shape['bias']) for c in cs) == set((a, b) for a in (0, 1, 4) for b in (0, 1))
    # a forced call is admitted whatever the tile count; the automatic route asks for two rounds of the resident workgroups
    assert G.stream_plan(128, 128, 128, 0, 128, 128, 128, 0, 512) is None and G.stream_plan(128, 128, 128, 0, 128, 128, 128, 2, 512)
    assert G.stream_plan(128 * 128, 1024, 128, 0, 128, 128, 1024, 0, 512)['xcd_map'] == 1
    for c in cs:            # nothing needs more than about 70 MB per operand
        assert max(c.shape['M'] * c.shape['ldc'], c.shape['M'] * c.shape['lda']) * 4 <= 70 << 20, c


def test_sliced_cases_reach_their_slice_counts():
    sk = G.cases('splitk')
    for route in ('splitk_fast', 'splitk_aligned', 'splitk_scalar'):
        mine = [c for c in sk if c.route == route]
        assert all(c.shape['M'] > 128 and c.plan['tiles'] < 128 for c in mine)
        assert set(c.plan['ns'] for c in mine) >= {2, 5, 7}, route              # 2; cut by K / s >= 128; K = 1056: 7 slices of 160
        assert any(c.plan['last'] < c.plan['kslice'] for c in mine), route
        assert set(c.shape['bias'] for c in mine) == {0, 1} and len(set(c.shape['act'] for c in mine)) >= 3
    fast = [c for c in sk if c.route == 'splitk_fast']
    assert any(c.plan['ns'] == 8 and c.plan['last_full'] for c in fast)         # the 8-slice cap
    assert any(c.shape['K'] == 1056 and (c.plan['ns'], c.plan['kslice'], c.plan['last']) == (7, 160, 96) for c in fast)
    assert any(c.plan['tiles'] == 126 for c in fast)
    assert any(c.plan['last'] == 1 for c in sk if c.route == 'splitk_scalar')
    assert any(c.plan['tiles'] >= 128 and c.plan['ns'] == 1 and c.route == 'plain_fast' for c in sk)
    assert G.splitk_choice_fill(2048, 768, 3072) == 5                          # the example of the source comment: 96 tiles, 5 slices
    ss = G.cases('skinny_sliced')
    for w in (16, 32, 64):
        mine = [c for c in ss if c.route == 'skinny_sliced%d' % w]
        assert any(c.plan['ns'] > 1 and c.plan['last_full'] for c in mine), w
        assert any(c.plan['ns'] > 1 and not c.plan['last_full'] for c in mine), w
        assert any(c.plan['ns'] == 1 for c in mine), w
    assert any(c.shape['N'] == 2048 and c.shape['K'] == 4096 and c.route == 'skinny_sliced64' for c in ss)
    assert G.skinny_plan(128, 4104, 1028) == (4, 192, 6, 68) and G.skinny_plan(128, 1024, 256) == (2, 128, 2, 128)
    # M = 80: five 16-row tiles, wave 0 multiplies two of them and waves 1-3 one
    assert any(c.shape['M'] == 80 for c in ss) and any(c.shape['M'] == 80 for c in G.cases('skinny_direct'))
    tn = G.cases('tn')
    for nsl in G.TN_NSL[1:]:
        mine = [c for c in tn if c.plan['nsl'] == nsl]
        assert mine and all(c.plan['last_short'] for c in mine if c.shape['R'] > 17), nsl
    for T in (32, 64, 128):
        for al in ('aligned', 'scalar'):
            mine = [c for c in tn if c.route == 'tn%d_%s' % (T, al)]
            assert any(c.plan['nsl'] >= 16 for c in mine) and any(c.plan['direct'] for c in mine), (T, al)
    assert any(c.shape['acc'] and c.plan['nsl'] == 1 for c in tn) and any(c.shape['acc'] and c.plan['nsl'] > 16 for c in tn)
    assert any(c.shape['colsum'] and c.plan['nsl'] > 16 for c in tn) and any(c.shape['colsum'] and c.plan['direct'] for c in tn)
    assert any(c.shape['ldc'] > c.shape['Q'] and c.plan['direct'] for c in tn) and any(c.shape['ldc'] > c.shape['Q'] and c.plan['nsl'] > 1 for c in tn)
    assert G.tn_plan(257, 32, 32) == (32, 2, 144, 113) and G.tn_plan(8193, 32, 32) == (32, 33, 256, 1)
    tb = G.cases('tn_batched')
    assert set(c.route for c in tb) >= {'tnb32_aligned', 'tnb32_scalar', 'tnb64_aligned', 'tnb128_scalar', 'tnb128_aligned'}
    assert any(c.shape['batch_a'] % 4 for c in tb) and any(c.shape['batch_b'] % 4 for c in tb)


@pytest.mark.parametrize("group", G.GROUPS)
def test_bound_sees_a_dropped_last_index(group):
    checked = 0
    for c in G.cases(group):
        x = c.inputs()
        bad = c.defect(x)
        if bad is None:
            assert c.reduced == 0
            continue
        ref = c.reference(x)
        bound = c.fallback(x) if c.rule == 'fallback' else None
        for name, d in bad.items():
            want, e32, tol = ref[name]
            assert torch.isfinite(want).all() and e32 == e32, (c, name)
            moved = (d - want).abs()
            if bound is None:
                ratio = float(moved.max()) / tol
            else:
                ratio = float((moved / bound[name].clamp_min(1e-300)).max())
            assert ratio >= G.SENSITIVITY, "%s %s: defect moves %.3g, %.3g x the %s bound (e32 %.3g)" % (c, name, float(moved.max()), ratio,
                                                                                                        c.rule, e32)
            checked += 1
    assert checked


def test_fallback_bound_holds_for_the_float32_reference_and_sees_the_defect():
    """The a-priori bound on the longest reduction of every group: the float32 CPU evaluation (an fp32 sum in SOME order) is inside
    it element by element, and the dropped last index is not."""
    for group in G.GROUPS:
        c = max((c for c in G.cases(group) if not c.shape.get('nan')), key=lambda c: (c.reduced, -c.shape.get('M', 0)))
        x = c.inputs()
        bound, bad = c.fallback(x), c.defect(x)
        w64, w32 = c.evaluate(x, torch.float64), c.evaluate(x, torch.float32)
        for name, want in w64.items():
            assert bool(((w32[name].double() - want).abs() <= bound[name]).all()), (c, name)
            assert float(((bad[name] - want).abs() / bound[name]).max()) >= G.SENSITIVITY, (c, name)


def test_fallback_names_are_cases():
    assert G.FALLBACK <= set(c.name for c in G.CASES)


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_constants_are_the_ones_of_the_source():
    """The mirrors' constants and thresholds, as the source text states them (whitespace folded)."""
    f32, stream, skinny, tn = _src("gemm_f32.hip"), _src("gemm_stream.hip"), _src("gemm_skinny.hip"), _src("gemm_tn.hip")
    assert "constexpr int BM = %d, BN = %d, BK = %d," % (G.BM, G.BN, G.BK) in f32
    assert "constexpr int GS_BM = %d," % G.GS_BM in stream
    assert "constexpr int SK_KC = %d, SK_MAXM = %d;" % (G.SK_KC, G.SK_MAXM) in skinny
    assert "constexpr int TN_RK = %d;" % G.TN_RK in tn and "constexpr int TN_MAXSLICES = %d;" % G.TN_MAXSLICES in tn
    pins = {
        "gemm_f32.hip": (
            # launch_gemm
            "const bool fast = aligned && g.group <= 1 && (g.K % BK == 0) && g.K >= BK && g.rows_per_tile == BM &&",
            "const unsigned grid = 8u * (unsigned)(per_xcd < 64 ? per_xcd : 64);",
            # the persistent walk
            "const int64_t q_ = ntile / 8, r_ = ntile % 8;",
            "for (int64_t tt = slot; tt < t_count; tt += nslots) {",
            # gemm_splitk_choice_fill and the ksplit rounding
            "if (tiles >= 128 || tiles < 1 || K < 256) return 1;",
            "int s_ = (int)(512 / tiles); if (s_ > 8) s_ = 8;",
            "while (s_ > 1 && K / s_ < 128) --s_; return s_ < 1 ? 1 : s_; }",
            "const int64_t ksplit = ceil_div(ceil_div(K, (int64_t)(splits > 1 ? splits : 1)), (int64_t)BK) * BK;",
            "const bool ok = splits > 1 && ns > 1 && (lda % 4 == 0) && (ldb % 4 == 0) && (K % BK == 0) && K >= BK &&",
            # itr_gemm_nt_splitk and gemm_nt_algo
            "if (M <= 128 && N >= 16 && K >= 128 && itr::gemm_skinny_ok(A, lda, B, ldb, M, N, K) && workspace &&",
            "if (N >= 64 && K >= 128 && gemm_skinny_ok(A, lda, B, ldb, M, N, K)) return gemm_skinny_direct(",
            "(BM / group) * group, nullptr,",
        ),
        "gemm_stream.hip": (
            "if ((act != 0 && act != 1 && act != 4) || K % 64 != 0 || K < 128 || N % GS_BM != 0 || M < GS_BM) return false;",
            "const int64_t min_rounds = algo >= 2 ? 0 : 2;",
            "if (tiles_m * tiles_n < min_rounds * resident) return false;",
            "int64_t grid = resident / tiles_n * tiles_n; if (grid < tiles_n) grid = tiles_n;",
            "const int xcd_map = (algo != 2 && tiles_n >= 4 && grid % 8 == 0 && (grid / 8) % tiles_n == 0) ? 1 : 0;",
            "const unsigned nw = __builtin_amdgcn_readfirstlane(gridDim.x / tiles_n);",
            "q_ = __builtin_amdgcn_readfirstlane(tiles_m / nw), r_ = __builtin_amdgcn_readfirstlane(tiles_m % nw);",
            "const int nk2 = g.K / 64;",
            "(2 on gfx950: 64 KB of LDS each)",
        ),
        "gemm_skinny.hip": (
            "return M >= 1 && M <= SK_MAXM && N >= 16 && K >= SK_KC && K % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 &&",
            "const int nc = (N >= 4096 || (N >= 2048 && K >= 4096)) ? 4 : (N >= 1024 ? 2 : 1);",
            "int64_t s = ceil_div((int64_t)(nc > 1 ? 512 : 384), col_tiles);",
            "const int64_t by_k = K / (2 * SK_KC) > 0 ? K / (2 * SK_KC) : 1;",
            "const int kslice = (int)(ceil_div(ceil_div(K, s), (int64_t)SK_KC) * SK_KC);",
            "const bool t0 = wave < rtiles, t1 = wave + 4 < rtiles;",
        ),
        "gemm_tn.hip": (
            "return m > 64 ? 128 : (m > 32 ? 64 : 32);",
            "constexpr int64_t target = 1024;",
            "const int64_t by_rows = ceil_div(R, (int64_t)256);",
            "int64_t rps = ceil_div(ceil_div(R, s), (int64_t)TN_RK) * TN_RK;",
            "for (; k + 16 <= nsl; k += 16) {",
            "const bool direct = nsl == 1 && !accumulate;",
        ),
    }
    text = {"gemm_f32.hip": f32, "gemm_stream.hip": stream, "gemm_skinny.hip": skinny, "gemm_tn.hip": tn}
    for name, lines in pins.items():
        for line in lines:
            assert line in text[name], "%s no longer says: %s" % (name, line)
