"""No GPU: the case table of the SGRAF evaluation sweep (tests/helpers/sgraf_eval_cases.py) is fit for its purpose.

References: the float64 mirror of the library's algebra is the oracle's function (1e-11), so its float32 run measures that algebra's
own rounding.  Conditions per case: (a) the sharpness figure of the module is >= 2, (b) the float64 scores span >= 0.05,
(c) 16 * max(e32_oracle, e32_mirror) <= 5e-6; tol <= 5e-6, never looser than the flat bound of the older tests.  Coverage: every
seam value of the driver keeps a case (stated here a second time), and taking the carriers of a value out of the table is noticed.
Sensitivity: each claimed defect moves S by at least 10 x the bound the GPU sweep applies.  Planner mirrors: held against hand-written
plans.  Pins: the constants the mirrors copy are checked against the source text of csrc/, include/ and ops.py, so an edit to the
driver's geometry fails here instead of silently moving the seams."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sgraf_eval_cases as G        # noqa: E402
import scan_train_cases as S        # noqa: E402
import train_prim_cases as P        # noqa: E402

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-text-retrieval_amd")

# what the table must hold, stated here a second time: an edit that shrinks SEAMS in the helper does not shrink the requirement
REQUIRED = {
    'route': ('saf256', 'saf_generic', 'sgr_fused', 'sgr_chain256', 'sgr_chain', 'sgr_non_persistent', 'sgr_fused_rows32'),
    'S_saf': (16, 48, 64, 80, 256, 1024), 'S_sgr': (16, 48, 64, 256, 1024), 'sgr_step': (1, 2, 3, 8), 'D': (32, 64, 96, 288, 1024),
    'Ni@256': (1, 3, 4, 5, 64, 65), 'Ni@other': (1, 4, 5, 9), 'image_block@Ni': [(ib, n) for ib in (4, 8, 64) for n in (9, 65)],
    'slabs': (('saf256', 2), ('sgr_chain', 2)), 'W': (1, 2, 3, 4), 'saf_tail': (0, 1, 2, 3), 'max_len': (15, 16, 31, 32, 47, 48, 63),
    'pair_kernels': ('<1>', '<2>', '<2>+<4>'), 'Nc': (1, 63, 64, 65, 129), 'glo_tiles': (1, 2, 3), 'pairs%4': ('nonzero',),
    'tiles': ('one', 'several', 'ncap16', 'fill64', '63+1'),
    'group_shape': ('16x2nodes', '17x1word', 'fill64rows', '32+15x1', '48+7x1', 'single'), 'ptiles': (23, 24),
    'n_groups': (1, 256, 257, 1024, 1025), 'two_classes': ('across1024',),
    'walk64': ('below', 'equal', 'above', 'twice'), 'walk32': ('below', 'equal', 'above', 'twice'),
    'long': (64, 82), 'out_given': (True,), 'zero': ('region', 'word'),
}


def missing(cs, required):
    seen = {}
    for c in cs:
        for k, vs in c.seams().items():
            seen.setdefault(k, set()).update(str(v) for v in vs)
    return [(k, v) for k, vs in required.items() for v in vs if str(v) not in seen.get(k, ())]


def test_every_seam_value_has_a_case():
    assert not missing(G.CASES, REQUIRED)
    assert not missing(G.CASES, G.SEAMS)
    for k, vs in REQUIRED.items():          # the helper's own list asks for no less
        assert set(str(v) for v in vs) <= set(str(v) for v in G.SEAMS[k]), k


def test_taking_out_the_carriers_of_a_value_is_noticed():
    """The mutation check: for every required value, the table without the cases that carry it fails the coverage on that value; and
    a good share of the values hang on one or two cases only, i.e. the table is not padded."""
    few = 0
    for k, vs in REQUIRED.items():
        for v in vs:
            carriers = [c.name for c in G.CASES if str(v) in set(str(s) for s in c.seams().get(k, ()))]
            assert carriers, (k, v)
            rest = [c for c in G.CASES if c.name not in carriers]
            assert (k, v) in missing(rest, REQUIRED), (k, v)
            few += len(carriers) <= 2
    assert few >= 40, few


def test_table_shapes_follow_the_rules():
    assert 100 <= len(G.CASES) <= 200 and len(set(c.name for c in G.CASES)) == len(G.CASES)
    for c in G.CASES:
        x = c.inputs()
        assert x['images'].shape == (c.Ni, 36, c.D) and x['words'].shape == (c.n_tok, c.D) and c.D % 32 == 0
        nrm_i, nrm_w = x['images'].norm(dim=-1), x['words'].norm(dim=-1)
        if c.zero is None:
            assert float((nrm_i - 1).abs().max()) < 1e-5 and float((nrm_w - 1).abs().max()) < 1e-5, c         # l2-normalised
        elif c.zero[0] == 'region':
            assert float(x['images'][c.zero[1][0], c.zero[1][1]].abs().max()) == 0.0 and int((nrm_i < 0.5).sum()) == 1
        else:
            assert float(x['words'][c.zero[1]].abs().max()) == 0.0 and int((nrm_w < 0.5).sum()) == 1
            assert c.zero[1] not in S._offsets(c.lens)              # inside a caption, not its first word
        # the smallest shapes that reach the seam: D = 32 and Ni <= 5 unless the seam is D or Ni
        assert c.D == 32 or c.group == 'D', c
        assert c.Ni <= 5 or c.group in ('Ni', 'block', 'slab', 'walk') or (c.group == 'Nc' and c.Nc == 1), c
        assert c.Ni * c.n_tok <= 64 * 9 * 63 or c.group == 'ngroups', c      # the largest: the walk over nine 63-word captions
        assert c.out_given == (max(c.lens) > G.MAX_WORDS)
        w = c.weights
        assert w['sim_tranloc_w.weight'].shape == (c.S, c.D) and all(v.dtype == torch.float32 for v in w.values())
    # the n_groups cases: captions of >= 33 words share no group, Ni = 2
    for c in G.cases('ngroups'):
        assert c.Ni == 2 and c.plan.n_groups == c.Nc and all(len(g) == 1 for g in c.plan.groups), c
    # the persistent-walk cases are built for 256 CUs: items = n_groups x 64 images against 256 (64-row class) / 512 (32-row class)
    got = {(c.tag, tuple(c.plan.walk().items())) for c in G.cases('walk')}
    assert got == {('large3', ((64, 'below'),)), ('large4', ((64, 'equal'),)), ('large5', ((64, 'above'),)), ('large9', ((64, 'twice'),)),
                   ('small7', ((32, 'below'),)), ('small8', ((32, 'equal'),)), ('small9', ((32, 'above'),)), ('small17', ((32, 'twice'),))}
    assert all(c.Ni == 64 and c.plan.blocks == [(0, 64)] for c in G.cases('walk'))
    # the two-class case across 1 024: the 30 small groups come first, the large ones run on to group 1 029
    c = [c for c in G.cases('ngroups') if c.group_rows == 32][0]
    assert c.plan.n_class == [30, 1000] and [m[3] for m in c.plan.meta[:31]] == [0] * 30 + [1]
    # the second bn_tanh slab starts inside the call: image 1820
    assert G.BN_SLAB // 36 == 1820 and all(c.Ni == 1821 and c.plan.slabs == 2 and c.Nc == 2 for c in G.cases('slab'))
    assert all(c.plan.slabs == 1 for c in G.CASES if c.group != 'slab')
    # the scales were chosen once: one recipe of (module, sim_dim, steps)
    assert G.scales('SAF', 256) == {'sim_eval_w': 4.0, 'attn_sim_w': 48.0} and G.scales('SAF', 64) == {'sim_eval_w': 2.0, 'attn_sim_w': 24.0}
    assert G.scales('SGR', 256, 3) == {'graph_query_w': 6.0, 'graph_key_w': 6.0, 'sim_eval_w': 10.0}
    assert G.scales('SGR', 16, 8)['sim_eval_w'] == 5.625 and G.scales('SAF', 1024)['attn_sim_w'] == 48.0
    assert G.scales('SGR', 256, 3, 32) == G.scales('SGR', 256, 3, 256) != G.scales('SGR', 256, 3, 1024) and len(G.RESEED) <= 8


def test_planner_mirrors_against_hand_written_plans():
    # 1. three captions of 5, 9 and 3 words: one group of 6 + 10 + 4 = 20 node rows, largest first; every graph one node tile
    p = G.Plan('SGR', 5, 32, 256, (5, 9, 3))
    assert p.groups == [[1, 0, 2]] and p.meta == [(20, 3, 3, 0)] and p.group_begin == [0, 3] and p.group_order == [1, 0, 2]
    assert (p.route, p.ib, p.last_block, p.blocks, p.NcP, p.glo_tiles, p.n_tiles, p.pair_kernels) == ('sgr_fused', 8, 8, [(0, 5)], 64, 1, 1, '')
    # 2. 32 + fifteen one-word captions + 40 + 22: 33 + 15 x 2 = 63 rows (exact fill cannot reach 64 with 16 graphs), 3 + 15 units,
    #    9 + 15 = 24 softmax tiles; the companions fill a group of 41 + 23 = 64 rows with 3 + 2 units and 9 + 4 tiles
    p = G.Plan('SGR', 5, 32, 256, (32,) + (1,) * 15 + (40, 22))
    assert p.groups == [[16, 17], [0] + list(range(1, 16))] and p.meta == [(64, 5, 13, 1), (63, 18, 24, 1)]
    #    ... and with sgr_group_rows = 32 the one-word captions and the 22-word one go first, into groups of <= 32 rows
    p = G.Plan('SGR', 5, 32, 256, (32,) + (1,) * 15 + (40, 22), group_rows=32)
    assert p.groups[0] == [17, 1, 2, 3, 4] and p.meta[0] == (31, 6, 8, 0) and p.groups[1] == list(range(5, 16)) and p.meta[1] == (22, 11, 11, 0)
    assert p.groups[2:] == [[16], [0]] and [m[3] for m in p.meta] == [0, 0, 1, 1] and p.n_class == [2, 2]
    # 3. captions of 64 and 82 words leave; chain at sim_dim 64: block of 4, two blocks for 5 images, <2> only for 12 words + 1
    p = G.Plan('SGR', 5, 32, 64, (5, 64, 9, 12, 82, 3, 7))
    assert (p.short_idx, p.long_idx, p.k_len, p.max_len) == ([0, 2, 3, 5, 6], [1, 4], [5, 9, 12, 3, 7], 12)
    assert (p.route, p.ib, p.last_block, p.blocks, p.pair_kernels, p.glo_tiles) == ('sgr_chain', 4, 4, [(0, 4), (4, 1)], '<1>', 0)
    assert p.groups == [[2, 1, 4, 0, 3]] and p.meta == [(41, 5, 5, 1)]
    # the image blocks and the pair kernels, on both sides of their edges
    assert [G.image_block(256, n) for n in (1, 4, 5, 9, 64, 65, 1821)] == [4, 4, 8, 12, 64, 64, 64]
    assert [G.image_block(256, 65, ib) for ib in (4, 8, 64)] == [4, 8, 64] and G.image_block(256, 9, 64) == 12 and G.image_block(64, 65, 64) == 4
    assert G.Plan('SAF', 65, 32, 256, (3,)).blocks == [(0, 64), (64, 1)] and G.Plan('SAF', 9, 32, 256, (3,), pinned=64).last_block == 64
    assert [G.pair_kernels(n) for n in (1, 15, 16, 31, 32, 47, 48, 63)] == ['<1>', '<1>', '<2>', '<2>', '<2>+<4>', '<2>+<4>', '<2>+<4>', '<2>+<4>']
    assert G.group_meta([0], [63]) == (64, 4, 16, 1) and G.group_meta([0], [31]) == (32, 2, 4, 0) and G.group_meta([0, 1], [16, 14]) == (32, 3, 5, 0)
    assert G.group_meta([0] + list(range(1, 8)), [48] + [1] * 7) == (63, 11, 23, 1)
    # every group of every case keeps the device's limits, and the groups partition the kernel's captions
    for c in G.CASES:
        p = c.plan
        assert sorted(p.group_order) == list(range(p.Nc_kernel)) and all(m[0] <= 64 and m[1] <= 24 and m[2] <= 24 for m in p.meta), c
        if c.group_rows == 32:
            assert all((m[3] == 0) == (m[0] <= 32) for m in p.meta), c


@pytest.fixture(scope="module")
def refs():
    return {c.name: c.reference() for c in G.CASES}


def test_mirror_is_the_oracles_function_and_the_conditions_hold(refs):
    for c in G.CASES:
        want, e_oracle, e_mirror, tol, agree, sharp = refs[c.name]
        m = float(want.abs().max())
        assert want.shape == (c.Ni, c.Nc) and bool(torch.isfinite(want).all()) and e_oracle == e_oracle and e_mirror == e_mirror, c
        assert agree <= G.MIRROR_AGREES, (c, agree)
        assert sharp >= G.MIN_SHARP, "%s: sharpness %.3g" % (c, sharp)                                            # (a)
        span = float(want.max() - want.min())
        assert span >= G.MIN_SPAN, "%s: the scores span %.3g" % (c, span)                                          # (b)
        assert G.FACTOR * max(e_oracle, e_mirror) <= G.OLD_BOUND, "%s: e32 oracle %.3g mirror %.3g" % (c, e_oracle, e_mirror)      # (c)
        if c.name not in G.FALLBACK:
            assert tol == G.FACTOR * max(e_oracle, e_mirror, G.U * m), c
        assert tol <= G.OLD_BOUND, "%s: tol %.3g is looser than the flat %.3g" % (c, tol, G.OLD_BOUND)
        # the float32 references themselves pass at ratio <= 1 / 16
        assert max(e_oracle, e_mirror) <= tol / G.FACTOR, c


def test_bound_sees_every_claimed_defect(refs):
    claimed = {}
    for c in G.CASES:
        want, tol = refs[c.name][0], refs[c.name][3]
        for letter, value in c.defects().items():
            assert value.shape == want.shape, (c, letter)
            moved = float((value - want).abs().max())
            assert moved >= G.SENSITIVITY * tol, "%s defect %s moves S by %.3g, %.3g x its bound" % (c, letter, moved, moved / tol)
            claimed.setdefault(letter, []).append(c)
    assert set(claimed) == set('abcskgtno')
    # the claims follow the rules of the helper's docstring, restated
    for c in G.CASES:
        p, big = c.plan, c.Nc > 1000 or c.Ni > 1000
        want = ''
        if not big:
            want += ('a' if c.D <= 96 else '') + 'b' + ('c' if max(c.lens) > 1 else '')
            want += 's' if any(p.k_len[t[k]] > 1 and p.k_len[t[k + 1]] < 63 for t in p.cols.tiles for k in range(len(t) - 1)) else ''
            want += 'k' if (c.mod == 'SGR' and any((n + 1) % 16 for n in c.lens)) or (c.mod == 'SAF' and c.S == 256 and any((n + 1) % 4 for n in c.lens)) else ''
            want += 'g' if c.Nc > 64 and not p.long_idx else ''
        want += 't' if c.Ni % 4 and c.Ni > 1 and c.Nc <= 1000 else ''
        want += 'n' if c.Ni * 36 > 65520 else ''
        want += 'o' if p.n_groups > 1024 and p.route == 'sgr_fused' else ''
        assert c.claims == want, (c, c.claims, want)
    assert set(c.Nc for c in claimed['g']) == {65, 129, 256, 257} and set(c.plan.n_groups for c in claimed['o']) == {1025, 1030}
    assert set(c.Ni for c in claimed['n']) == {1821} and set(c.Ni for c in claimed['t']) >= {3, 5, 9, 65, 1821}
    assert set(c.route_name() for c in claimed['k']) == set(REQUIRED['route']) - {'saf_generic'}


def test_fallback_list():
    assert set(G.FALLBACK) <= set(c.name for c in G.CASES)
    assert len(G.FALLBACK) <= G.FALLBACK_SHARE * len(G.CASES)
    assert G.FALLBACK_SHARE == 0.02 and G.FACTOR == P.FACTOR == 16 and G.U == P.U == 2.0 ** -24 and G.SENSITIVITY == P.SENSITIVITY == 10
    assert G.MIRROR_AGREES == S.MIRROR_AGREES == 1e-11 and G.OLD_BOUND == 5e-6 and (G.MIN_SPAN, G.MIN_SHARP) == (0.05, 2.0)
    assert all(v <= G.OLD_BOUND for v in G.FALLBACK.values())


def _src(*path):
    with open(os.path.join(PKG, *path)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_constants_are_the_ones_of_the_source():
    """The mirrors' constants and gates, as the source text states them (whitespace folded)."""
    text = {"sgraf.hip": _src("csrc", "sgraf.hip"), "sgr_fused.hip": _src("csrc", "sgr_fused.hip"), "scan_common.h": _src("csrc", "scan_common.h"),
            "ops.py": _src("itr_amd", "ops.py"), "itr_hip.h": _src("..", "include", "itr_hip.h")}
    pins = {
        "scan_common.h": ("constexpr int SC_R = %d;" % G.SC_R, "constexpr int SC_IMGS = %d;" % G.SC_IMGS, "constexpr int SC_NT = ITR_SCAN_NT;"),
        "itr_hip.h": ("#define ITR_SCAN_NT %d" % G.SC_NT, "#define ITR_SGRAF_DEFAULT_IMAGE_BLOCK %d" % G.DEFAULT_BLOCK,
                      "#define ITR_SGRAF_UNFUSED_STEPS 1", "#define ITR_SGRAF_NON_PERSISTENT 2"),
        "sgr_fused.hip": (
            "constexpr int SF_ROWS = %d, SF_S = 256, SF_LD = 260, SF_MAXCAP = %d, SF_MAXUNIT = %d," % (G.SF_ROWS, G.SF_MAXCAP, G.SF_MAXUNIT),
            "constexpr int SF_SMALL = %d;" % G.SF_SMALL,
            "constexpr int sf_ptiles(int rows) { return rows > SF_SMALL ? %d : %d; }" % (G.SF_PTILES[64], G.SF_PTILES[32]),
            # the group records
            "const int64_t gi = (int64_t)blockIdx.x * %d + threadIdx.x;" % G.META_BLOCK,
            "dim3((unsigned)ceil_div(n_groups, %d)), dim3(%d), 0, st, grp_begin, grp_order, cap_len, cap_col," % (G.META_BLOCK, G.META_BLOCK),
            "if ((m.nn[s] + 15) / 16 == nt) for (int b = 0; b < nt; ++b)", "po += (m.nn[m.unit_cap[u]] + 15) / 16; }",
            "if (po > sf_ptiles(SF_ROWS)) { refuse(); return; }", "const bool small = rows <= SF_SMALL && po <= sf_ptiles(SF_SMALL);",
            # the class lists
            "for (int64_t g0 = 0; g0 < n_groups; g0 += %d) {" % G.CLASSIFY_CHUNK,
            "hipLaunchKernelGGL(sgr_group_classify_kernel, dim3(1), dim3(%d), 0, st, w.cls, n_groups, w.glist, w.gcount);" % G.CLASSIFY_CHUNK,
            # the persistent walk
            "const int64_t grid = n_groups * g.nb;", "const int64_t resident = cus * WG_PER_CU;", "dim3((unsigned)(grid < resident ? grid : resident))",
            "int rc = sgr_fused_launch_class<SF_ROWS, %d>(g, 1, n_groups, w, persistent, st);" % G.WG_PER_CU[64],
            "return sgr_fused_launch_class<SF_SMALL, %d>(g, 0, n_groups, w, persistent, st);" % G.WG_PER_CU[32],
            # the planner
            "for (int pass = (small_rows == SF_ROWS ? 1 : 0); pass < 2; ++pass) {",
            "const int cap_rows = pass == 0 ? SF_SMALL : SF_ROWS, lo = (pass == 0 || small_rows == SF_ROWS) ? 2 : SF_SMALL + 1;",
            "if (n >= lo && n <= cap_rows) by_n[n].push_back((int32_t)c);", "pack_bins(by_n, cap_rows, SF_MAXCAP, bins);",
        ),
        "sgraf.hip": (
            "for (int64_t r0 = 0; r0 < Ni * SC_R; r0 += %d) {" % G.BN_SLAB, "const int64_t nr = (Ni * SC_R - r0 < %d) ? Ni * SC_R - r0 : %d;" % (G.BN_SLAB, G.BN_SLAB),
            "if (S != 256) return %d;" % G.OTHER_BLOCK, "int64_t ib = image_block > 0 ? image_block : ITR_SGRAF_DEFAULT_IMAGE_BLOCK;",
            "const int64_t need = (Ni + SC_IMGS - 1) / SC_IMGS * SC_IMGS;", "return ib < SC_IMGS ? SC_IMGS : ib;",
            "const int64_t NcP = (Nc + SC_NT - 1) / SC_NT * SC_NT;", "const bool glo_loc = S == 256;",
            "const int64_t pair = (int64_t)blockIdx.x * %d + (threadIdx.x >> 6);" % G.PAIRS_PER_WG,
            "const int ntmax = (max_len + 1 + 15) / 16;", "if (ntmax == 1) {", "if (ntmax > 2) {",
            "const int n = n0 + k < nn ? n0 + k : nn - 1;", "if (p.S == 256) {", "float vec[16];",
            "ITR_UNSUPPORTED(S > %d || (D %% SC_BK) != 0," % G.MAX_S, "ITR_UNSUPPORTED(module == 1 && (sgr_step < 1 || sgr_step > %d)," % G.MAX_STEPS,
            "ITR_UNSUPPORTED(S % 16 != 0, \"itr_sgraf_scores: SGR needs sim_dim %% 16 == 0\");",
            "static inline bool sgraf_fused_layout(int module, int S, int flags) { return module == 1 && S == 256 && !(flags & ITR_SGRAF_UNFUSED_STEPS); }",
            "per block of 64 images",
        ),
        "ops.py": ("SGRAF_MAX_WORDS = %d " % G.MAX_WORDS, 'SGRAF_FLAGS = {"unfused_steps": 1, "non_persistent": 2}',
                   "small = 32 if SETTINGS.sgr_group_rows == 32 else SCAN_NT", "out[:, torch.from_numpy(plan.short_idx).to(dev)] = part"),
    }
    for name, lines in pins.items():
        for line in lines:
            assert line in text[name], "%s no longer says: %s" % (name, line)
